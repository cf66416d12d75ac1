"""The arguments of tl.cnv_copy_segments and of the six entry points behind it that are refused before any GPU work: the
exception's type (the entry's status) and the rule it names.  No test here needs a device."""
import ctypes

import numpy as np
import pandas as pd
import pytest

INVALID, UNSUPPORTED = 1, 2  # ICV_ERR_INVALID, ICV_ERR_UNSUPPORTED
ONE = ctypes.c_void_p(16)    # never dereferenced: every call below fails in the argument checks


def _adata(S=None, chr_pos=None, P=None, obs=None):
    from infercnvpy_amd._compat import SimpleAnnData

    S = np.zeros((4, 10), dtype=np.int8) if S is None else S
    ad = SimpleAnnData(np.zeros((S.shape[0], 2), dtype=np.float32), obs=obs)
    ad.obsm["X_cnv_copy_states"] = S
    if P is not None:
        ad.obsm["X_cnv_copy_posterior_neutral"] = P
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def _no_levels():
    ad = _adata()
    del ad.obsm["X_cnv_copy_states"]
    return ad


def _no_chr_pos():
    ad = _adata()
    del ad.uns["cnv"]["chr_pos"]
    return ad


def _stored(params):
    ad = _adata()
    ad.uns["cnv_copy_states"] = {"params": params}
    return ad


CASES = [
    ("no_levels", _no_levels, {}, KeyError, "X_cnv_copy_states not found in adata.obsm. Did you run `tl.cnv_copy_states`"),
    ("no_chr_pos", _no_chr_pos, {}, KeyError, "chr_pos not found in adata.uns['cnv']"),
    ("not_2d", lambda: _adata(np.zeros(10, dtype=np.int8)), {}, ValueError, "X_cnv_copy_states must be 2-D"),
    ("not_int8", lambda: _adata(np.zeros((4, 10), dtype=np.int16)), {}, ValueError, "must be int8"),
    ("empty", lambda: _adata(np.zeros((0, 10), dtype=np.int8)), {}, ValueError, "empty matrix"),
    ("chr_pos_beyond", lambda: _adata(chr_pos={"a": 0, "b": 10}), {}, ValueError,
     "tl.cnv_copy_segments: chr_pos start 10 is outside [0, 10)"),
    ("min_fraction_0", _adata, {"min_fraction": 0}, ValueError, "tl.cnv_copy_segments: min_fraction=0 must lie in (0, 1]"),
    ("min_windows_0", _adata, {"min_windows": 0}, ValueError, "tl.cnv_copy_segments: min_windows=0 must be an integer >= 1"),
    ("range_lo", _adata, {"level_range": (-8, 0)}, ValueError, "level_range=(-8, 0) must satisfy -7 <= lo <= 0 <= hi <= 7"),
    ("range_hi", _adata, {"level_range": (0, 8)}, ValueError, "level_range=(0, 8) must satisfy"),
    ("range_without_0", _adata, {"level_range": (1, 3)}, ValueError, "level_range=(1, 3) must satisfy"),
    ("range_not_integers", _adata, {"level_range": (-1.5, 2)}, ValueError, "must be a pair of integers (lo, hi)"),
    ("range_not_a_pair", _adata, {"level_range": 3}, ValueError, "must be a pair of integers (lo, hi)"),
    ("range_of_a_stored_model_beyond_7", lambda: _stored({"levels": [0.1 * s for s in range(9)], "neutral": 0}), {},
     ValueError, "level_range=(0, 8) must satisfy"),
    ("no_groupby_column", _adata, {"groupby": "clone"}, ValueError, "`clone` not found in `adata.obs`"),
    ("plane_shape", lambda: _adata(P=np.zeros((4, 9))), {}, ValueError,
     "X_cnv_copy_posterior_neutral has shape (4, 9), X_cnv_copy_states has (4, 10)"),
    ("plane_dtype", lambda: _adata(P=np.zeros((4, 10), dtype=np.float32)), {}, ValueError,
     "X_cnv_copy_posterior_neutral must be float64, not float32"),
]


@pytest.mark.parametrize("make, kw, exc, message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_the_public_function_refuses_before_any_gpu_work(make, kw, exc, message):
    import infercnvpy_amd as cnv

    ad = make()
    kw = dict(kw)
    with pytest.raises(exc) as e:
        cnv.tl.cnv_copy_segments(ad, kw.pop("groupby", None), **kw)
    assert message in str(e.value)
    assert "cnv_copy_segments" not in ad.uns


def test_it_is_exported():
    import infercnvpy_amd as cnv

    assert "cnv_copy_segments" in cnv.tl.__all__ and callable(cnv.tl.cnv_copy_segments)
    ad = _adata(obs=pd.DataFrame({"clone": list("aabb")}))
    with pytest.raises(ValueError, match="level_range"):
        cnv.tl.cnv_copy_segments(ad, "clone", level_range=(0, -1))


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def _call(entry, **kw):
    """(status, message) of one call of ``entry``; every pointer is ONE unless ``missing`` names it."""
    from infercnvpy_amd import _lib

    lib = _lib.load()
    a = dict(n_rows=4, n_cols=10, n_chr=2, lo=-2, hi=3, n_seg=5, n_groups=2, n_listed=4, missing=None)
    a.update(kw)
    p = lambda name: None if a["missing"] == name else ONE  # noqa: E731
    if entry == "icv_level_segments_count":
        args = (p("states"), a["n_rows"], a["n_cols"], p("chr_start"), a["n_chr"], a["lo"], a["hi"], p("counts"), p("bad"))
    elif entry == "icv_level_segments_fill":
        args = (p("states"), a["n_rows"], a["n_cols"], p("chr_start"), a["n_chr"], p("offsets"), a["n_seg"], p("seg_row"),
                p("seg_start"), p("seg_end"), p("seg_level"))
    elif entry == "icv_level_votes":
        args = (p("states"), a["n_rows"], a["n_cols"], p("rows"), a["n_listed"], p("group_ptr"), a["n_groups"], a["lo"],
                a["hi"], p("counts"), p("bad"))
    elif entry == "icv_level_consensus":
        args = (p("counts"), p("need"), a["n_groups"], a["n_cols"], a["lo"], a["hi"], p("loss"), p("gain"), p("consensus"))
    elif entry == "icv_level_segments_support":
        args = (p("seg_row"), p("seg_start"), p("seg_end"), p("seg_level"), a["n_seg"], p("counts"), p("loss"), p("gain"),
                a["n_groups"], a["n_cols"], a["lo"], a["hi"], p("cells_min"), p("cells_sum"), p("level_min"), p("level_sum"))
    else:
        args = (p("p_neutral"), a["n_rows"], a["n_cols"], p("seg_row"), p("seg_start"), p("seg_end"), a["n_seg"], p("psum"),
                p("bad"))
    rc = getattr(lib, entry)(*args, None)
    return rc, lib.icv_last_error().decode()


POINTERS = {
    "icv_level_segments_count": ("states", "chr_start", "counts", "bad"),
    "icv_level_segments_fill": ("states", "chr_start", "offsets", "seg_row", "seg_start", "seg_end", "seg_level"),
    "icv_level_votes": ("states", "rows", "group_ptr", "counts", "bad"),
    "icv_level_consensus": ("counts", "need", "loss", "gain", "consensus"),
    "icv_level_segments_support": ("seg_row", "seg_start", "seg_end", "seg_level", "counts", "loss", "gain", "cells_min",
                                   "cells_sum", "level_min", "level_sum"),
    "icv_segments_psum": ("p_neutral", "seg_row", "seg_start", "seg_end", "psum", "bad"),
}
WITH_RANGE = ("icv_level_segments_count", "icv_level_votes", "icv_level_consensus", "icv_level_segments_support")


@pytest.mark.parametrize("entry", list(POINTERS))
def test_an_entry_refuses_null_pointers_and_bad_shapes(entry):
    who = entry[len("icv_"):]
    for name in POINTERS[entry]:
        assert _call(entry, missing=name) == (INVALID, f"{who}: a null pointer"), name
    rc, message = _call(entry, n_cols=0)
    assert rc == INVALID and message.startswith(f"{who}: n_") and "n_cols >= 1" in message
    negative = {"icv_level_consensus": "n_groups", "icv_level_segments_support": "n_seg"}.get(entry, "n_rows")
    rc, message = _call(entry, **{negative: -1})
    assert rc == INVALID and ">= 0" in message
    if entry in ("icv_level_segments_count", "icv_level_segments_fill"):
        for n_chr in (0, 11, -1):
            assert _call(entry, n_chr=n_chr) == (INVALID, f"{who}: 1 <= n_chr <= n_cols")
    if entry in WITH_RANGE:
        for lo, hi in ((-8, 0), (0, 8), (1, 2), (-2, -1)):
            assert _call(entry, lo=lo, hi=hi) == (INVALID, f"{who}: the level range ({lo}, {hi}) breaks -7 <= lo <= 0 <= hi <= 7")
    if entry == "icv_segments_psum":
        rc, message = _call(entry, n_cols=(1 << 22) + 1)
        assert rc == UNSUPPORTED and message == "segments_psum: n_cols = 4194305 is above 4194304 (the int64 sum of a run)"


def test_the_level_bound_is_the_librarys():
    from infercnvpy_amd import _lib

    assert _lib.ICV_LEVEL_MAX == 7 and _lib.ICV_FILTER_MAX_WINDOWS == 1 << 22

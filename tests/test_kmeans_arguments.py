"""The arguments of tl.cnv_kmeans and of the five entry points behind it that are refused before any GPU work: the
exception's type and the rule it names.  No test here needs a device."""
import ctypes

import numpy as np
import pytest

INVALID = 1                # ICV_ERR_INVALID
ONE = ctypes.c_void_p(16)  # never dereferenced: every call below fails in the argument checks


def _adata(x=None):
    from infercnvpy_amd._compat import SimpleAnnData

    x = np.random.default_rng(0).normal(0, 1, (6, 3)).astype(np.float32) if x is None else x
    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
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


def _init_with(value):
    init = np.zeros((2, 3))
    init[1, 2] = value
    return init


CASES = [
    ("k_1", _adata, {"n_clusters": 1}, ValueError, "`n_clusters` must be at least 2, got 1"),
    ("k_0", _adata, {"n_clusters": 0}, ValueError, "`n_clusters` must be at least 2, got 0"),
    ("k_257", lambda: _adata(np.zeros((300, 2))), {"n_clusters": 257}, ValueError, "`n_clusters` must be at most 256, got 257"),
    ("k_above_n", _adata, {"n_clusters": 7}, ValueError, "`n_clusters` = 7 exceeds the 6 rows of X_cnv_pca"),
    ("k_float", _adata, {"n_clusters": 2.0}, TypeError, "`n_clusters` must be an integer, got 2.0"),
    ("k_bool", _adata, {"n_clusters": True}, TypeError, "`n_clusters` must be an integer"),
    ("n_init_float", _adata, {"n_clusters": 2, "n_init": 1.5}, TypeError, "`n_init` must be an integer, got 1.5"),
    ("n_init_0", _adata, {"n_clusters": 2, "n_init": 0}, ValueError, "`n_init` must be at least 1, got 0"),
    ("max_iter_str", _adata, {"n_clusters": 2, "max_iter": "3"}, TypeError, "`max_iter` must be an integer, got '3'"),
    ("max_iter_0", _adata, {"n_clusters": 2, "max_iter": 0}, ValueError, "`max_iter` must be at least 1, got 0"),
    ("random_state_float", _adata, {"n_clusters": 2, "random_state": 0.5}, TypeError, "`random_state` must be an integer"),
    ("init_shape", _adata, {"n_clusters": 2, "init": np.zeros((3, 3))}, ValueError,
     "`init` must be \"k-means++\" or an array of shape (2, 3), got (3, 3)"),
    ("init_components", _adata, {"n_clusters": 2, "init": np.zeros((2, 4))}, ValueError, "got (2, 4)"),
    ("init_1d", _adata, {"n_clusters": 2, "init": np.zeros(6)}, ValueError, "got (6,)"),
    ("init_name", _adata, {"n_clusters": 2, "init": "random"}, ValueError, "got 'random'"),
    ("init_nan", _adata, {"n_clusters": 2, "init": _init_with(np.nan)}, ValueError, "`init` has non-finite values"),
    ("init_inf", _adata, {"n_clusters": 2, "init": _init_with(np.inf)}, ValueError, "`init` has non-finite values"),
    ("nan", lambda: _with(np.nan), {"n_clusters": 2}, ValueError, "X_cnv_pca has non-finite values"),
    ("inf", lambda: _with(-np.inf), {"n_clusters": 2}, ValueError, "X_cnv_pca has non-finite values"),
    ("too_many_components", lambda: _adata(np.zeros((6, 257))), {"n_clusters": 2}, ValueError,
     "X_cnv_pca has 257 components; at most 256 are supported"),
    ("no_components", lambda: _adata(np.zeros((6, 0))), {"n_clusters": 2}, ValueError, "empty matrix of shape (6, 0)"),
    ("no_representation", _no_rep, {"n_clusters": 2}, KeyError,
     "tl.cnv_kmeans: X_cnv_pca not found in adata.obsm. Did you run `tl.pca`?"),
    ("other_rep", _adata, {"n_clusters": 2, "use_rep": "umap"}, KeyError, "X_umap not found in adata.obsm"),
    ("shift_below_0", lambda: _with(2.0 ** 40), {"n_clusters": 2}, ValueError, "too large for exact int64 sums: rescale X_cnv_pca"),
    ("init_shift_below_0", _adata, {"n_clusters": 2, "init": _init_with(2.0 ** 40)}, ValueError, "rescale X_cnv_pca"),
]


@pytest.mark.parametrize("name,make,kwargs,exc,text", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_come_before_any_gpu_work(name, make, kwargs, exc, text):
    import infercnvpy_amd as cnv

    ad = make()
    with pytest.raises(exc) as info:
        cnv.tl.cnv_kmeans(ad, **kwargs)
    assert text in str(info.value)
    assert "cnv_kmeans" not in ad.obs.columns and "cnv_kmeans" not in ad.uns


def test_cnv_kmeans_is_public():
    import infercnvpy_amd as cnv

    assert "cnv_kmeans" in cnv.tl.__all__ and callable(cnv.tl.cnv_kmeans)


def test_shifts_and_draws_are_the_oracles():
    import _kmeans_oracle as ko
    from infercnvpy_amd import _lib
    from infercnvpy_amd.tl import _kmeans

    assert (_lib.ICV_KMEANS_MAX_CLUSTERS, _lib.ICV_KMEANS_MAX_COMPONENTS, _lib.ICV_KMEANS_MAX_SHIFT) == \
        (ko.MAX_CLUSTERS, ko.MAX_COMPONENTS, ko.MAX_SHIFT)
    for m in (0.0, 1e-300, 0.5, 1.0, 3.7, 2047.9, 2.0 ** 20, 2.0 ** 30, 2.0 ** 45):
        for n in (2, 66, 4095, 10 ** 6):
            for c in (1, 2, 3, 50, 255, 256):
                assert _kmeans.shifts(m, n, c) == ko.shifts(m, n, c)
    for seed in (0, 1, -1, 2 ** 63 - 1, -(2 ** 63)):
        got = _kmeans.draws(seed, 3, 5)
        assert got == [[ko.mix(ko.run_base(seed, r) ^ t) for t in range(5)] for r in range(3)]


def test_constants_are_the_headers():
    import os
    import re

    from infercnvpy_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "infercnv_hip.h")).read()
    defined = dict(re.findall(r"#define (ICV_KMEANS_\w+) (\d+)", header))
    assert len(defined) == 9
    for name, value in defined.items():
        assert getattr(_lib, name) == int(value)
    for name in ("icv_kmeans_seed_dist", "icv_kmeans_seed_pick", "icv_kmeans_assign", "icv_kmeans_update",
                 "icv_kmeans_centres"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.EXPORTS and getattr(_lib.load(), name).argtypes


MATRIX = dict(x=ONE, dtype=0, n_rows=10, n_comp=4, ld=4)
MATRIX_BAD = [("dtype", {"dtype": 2}), ("no_rows", {"n_rows": 0}), ("no_components", {"n_comp": 0}),
              ("components", {"n_comp": 257}), ("ld", {"ld": 3}), ("null_x", {"x": None})]
ENTRIES = {
    "icv_kmeans_seed_dist": (dict(MATRIX, centre=ONE, first=1, shift_f=40, mind=ONE, w=ONE, partials=ONE, flags=ONE),
                             MATRIX_BAD + [("shift_41", {"shift_f": 41}), ("shift_negative", {"shift_f": -1}),
                                           ("null_centre", {"centre": None}), ("null_mind", {"mind": None}),
                                           ("null_w", {"w": None}), ("null_partials", {"partials": None}),
                                           ("null_flags", {"flags": None})]),
    "icv_kmeans_seed_pick": (dict(MATRIX, w=ONE, partials=ONE, t=1, n_clusters=3, z=5, centres=ONE, picks=ONE, flags=ONE),
                             MATRIX_BAD + [("t_negative", {"t": -1}), ("t_is_k", {"t": 3}), ("k_0", {"n_clusters": 0, "t": 0}),
                                           ("k_257", {"n_clusters": 257}), ("null_w", {"w": None}),
                                           ("null_partials", {"partials": None}), ("null_centres", {"centres": None}),
                                           ("null_picks", {"picks": None}), ("null_flags", {"flags": None})]),
    "icv_kmeans_assign": (dict(MATRIX, centres=ONE, n_clusters=3, shift_f=40, labels=ONE, sqdist=ONE, stats=ONE, flags=ONE),
                          MATRIX_BAD + [("k_0", {"n_clusters": 0}), ("k_257", {"n_clusters": 257}),
                                        ("shift_41", {"shift_f": 41}), ("shift_negative", {"shift_f": -1}),
                                        ("null_centres", {"centres": None}), ("null_labels", {"labels": None}),
                                        ("null_sqdist", {"sqdist": None}), ("null_stats", {"stats": None}),
                                        ("null_flags", {"flags": None})]),
    "icv_kmeans_update": (dict(MATRIX, labels=ONE, n_clusters=3, shift_e=40, sums=ONE),
                          MATRIX_BAD + [("k_0", {"n_clusters": 0}), ("k_257", {"n_clusters": 257}),
                                        ("shift_41", {"shift_e": 41}), ("shift_negative", {"shift_e": -1}),
                                        ("null_labels", {"labels": None}), ("null_sums", {"sums": None})]),
    "icv_kmeans_centres": (dict(sums=ONE, n_clusters=3, n_comp=4, shift_e=40, centres=ONE),
                           [("k_0", {"n_clusters": 0}), ("k_257", {"n_clusters": 257}), ("no_components", {"n_comp": 0}),
                            ("components", {"n_comp": 257}), ("shift_41", {"shift_e": 41}),
                            ("shift_negative", {"shift_e": -1}), ("null_sums", {"sums": None}),
                            ("null_centres", {"centres": None})]),
}
ENTRY_CASES = [(entry, name, change) for entry, (_, bad) in ENTRIES.items() for name, change in bad]


@pytest.mark.parametrize("entry,name,change", ENTRY_CASES, ids=[f"{c[0][11:]}-{c[1]}" for c in ENTRY_CASES])
def test_entries_refuse_bad_arguments(entry, name, change):
    from infercnvpy_amd import _lib

    args = dict(ENTRIES[entry][0], **change)
    assert getattr(_lib.load(), entry)(*args.values(), None) == INVALID
    assert entry[4:].encode() in _lib.load().icv_last_error()

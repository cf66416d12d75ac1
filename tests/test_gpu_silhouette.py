"""tl.cnv_silhouette on the GPU equals the oracle of DESIGN.md 4.26 (tests/_silhouette_oracle.py) on the float64 bytes of
s, a and b and the codes of nearest: every storage of the representation and of the labels, the sizes at which the kernel
takes another path (the i- and j-tiles, the component stages, the chunks, the row slabs of S, the two forms of the
rounding) and the arithmetic pins."""
import functools

import numpy as np
import pandas as pd
import pytest

import _silhouette_oracle as so

pytestmark = pytest.mark.gpu

TILE = 64      # _engine.SILHOUETTE_TILE_I == SILHOUETTE_TILE_J (asserted below)
STAGE = 32     # _engine.SILHOUETTE_TILE_C


def points(n, c, seed, scale=1.0, dtype=np.float32):
    return (np.random.default_rng(seed).normal(0.0, 1.0, (n, c)) * scale).astype(dtype)


def random_codes(n, g, seed, missing=0.0):
    """Codes in which every one of the g groups has a cell (n >= g); a share ``missing`` of the cells has no label."""
    rng = np.random.default_rng(seed)
    codes = np.concatenate([np.arange(g), rng.integers(0, g, n - g)])
    rng.shuffle(codes)
    codes[rng.random(n) < missing] = -1
    return codes.astype(np.int64)


def widths(x, codes, n_groups, **kw):
    from infercnvpy_amd.tl._silhouette import silhouette_widths

    return silhouette_widths(x, codes, n_groups, **kw)


def same(got, want):
    """The float64 bytes of s, a, b and the codes of nearest."""
    for name in ("s", "a", "b"):
        assert got[name].dtype == np.float64
        assert got[name].tobytes() == want[name].tobytes(), name
    assert got["nearest"].dtype == np.int32 and got["nearest"].tolist() == want["nearest"].tolist()
    assert got["shift"] == want["shift"]


def check(x, codes, n_groups=None, **kw):
    g = int(codes.max()) + 1 if n_groups is None else n_groups
    host = x.cpu().numpy() if hasattr(x, "cpu") else x
    want = so.silhouette(np.asarray(host, dtype=np.float64), codes, g)
    got = widths(x, codes, g, **kw)
    same(got, want)
    return got, want


def test_tile_constants():
    from infercnvpy_amd import _engine

    assert (_engine.SILHOUETTE_TILE_I, _engine.SILHOUETTE_TILE_J, _engine.SILHOUETTE_TILE_C) == (TILE, TILE, STAGE)


# ---- storage ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def storage_case():
    x = points(150, 7, 1)
    codes = random_codes(150, 4, 2, missing=0.1)
    return x, codes, so.silhouette(x.astype(np.float64), codes, 4)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


STORAGE = {
    "host_f32": lambda x: x,
    "host_f64": lambda x: x.astype(np.float64),
    "host_f_ordered": lambda x: np.asfortranarray(x),
    "host_view": lambda x: np.repeat(np.repeat(x, 2, axis=0), 3, axis=1)[::2, ::3],
    "cuda_f32": lambda x: _cuda(x),
    "cuda_f64": lambda x: _cuda(x.astype(np.float64)),
    "cuda_view": lambda x: _cuda(np.repeat(np.repeat(x, 2, axis=0), 3, axis=1))[::2, ::3],
    "cuda_transposed": lambda x: _cuda(x.T.copy()).T,
}


@pytest.mark.parametrize("kind", list(STORAGE))
def test_every_storage_of_the_representation_gives_the_same_bytes(kind):
    x, codes, want = storage_case()
    stored = STORAGE[kind](x)
    if kind in ("host_view", "cuda_view"):
        assert not (stored.flags["C_CONTIGUOUS"] if isinstance(stored, np.ndarray) else stored.is_contiguous())
    same(widths(stored, codes, 4), want)


def test_float64_values_and_other_dtypes():
    x = np.random.default_rng(5).normal(0, 1, (90, 5))  # (float64 values that float32 cannot hold)
    codes = random_codes(90, 3, 6)
    check(x, codes)
    check(_cuda(x), codes)
    h = x.astype(np.float16)
    same(widths(h, codes, 3), so.silhouette(h.astype(np.float64), codes, 3))
    k = np.round(x * 10).astype(np.int32)
    same(widths(k, codes, 3), so.silhouette(k.astype(np.float64), codes, 3))


def _adata(x, column):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32), obs=pd.DataFrame({"cnv_leiden": column}))
    ad.obsm["X_cnv_pca"] = x
    return ad


@pytest.mark.parametrize("kind", ["categorical_unused", "strings", "strings_nan", "integers", "cuda"])
def test_every_storage_of_the_labels(kind):
    import infercnvpy_amd as cnv

    x, codes, _ = storage_case()
    names = np.array(["n", "t1", "t2", "t3"], dtype=object)
    if kind == "categorical_unused":
        cats = ["ghost", "n", "t1", "t2", "t3", "none"]
        column = pd.Categorical.from_codes(np.where(codes < 0, -1, codes + 1), categories=cats)
        want_codes, labels = np.where(codes < 0, -1, codes + 1), cats
    elif kind == "integers":
        c2 = np.where(codes < 0, 0, codes)  # (no missing label)
        column = (c2 * 10 + 7).tolist()
        order = pd.factorize(np.asarray(column))[0]
        want_codes, labels = order, list(pd.factorize(np.asarray(column))[1])
    else:
        column = np.where(codes < 0, None, names[np.maximum(codes, 0)]).astype(object)
        if kind == "strings":
            column = np.where(codes < 0, "t3", column).astype(object)
        want_codes, uniques = pd.factorize(column, use_na_sentinel=True)
        labels = list(uniques)
    want = so.silhouette(x.astype(np.float64), want_codes, len(labels))
    ad = _adata(_cuda(x) if kind == "cuda" else x, column)
    out = cnv.tl.cnv_silhouette(ad, return_info=True)
    s, nearest, info = out
    assert s.tobytes() == want["s"].tobytes() and nearest.tolist() == want["nearest"].tolist()
    assert info["a"].tobytes() == want["a"].tobytes() and info["b"].tobytes() == want["b"].tobytes()
    assert info["shift"] == want["shift"] == 40 and info["stage_ms"]["widths"] > 0
    assert ad.obs["cnv_silhouette"].to_numpy().tobytes() == want["s"].tobytes()
    col = ad.obs["cnv_silhouette_nearest"]
    assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == labels
    assert col.cat.codes.tolist() == want["nearest"].tolist()
    assert col.isna().to_numpy().tolist() == (want_codes < 0).tolist()
    uns = ad.uns["cnv_silhouette"]
    assert (uns["groupby"], uns["use_rep"], uns["shift"]) == ("cnv_leiden", "cnv_pca", 40)
    assert uns["mean"] == want["mean"]
    assert list(uns["groups"].index) == labels and uns["groups"]["n_cells"].tolist() == want["sizes"].tolist()
    assert uns["groups"]["mean"].to_numpy().tobytes() == want["group_mean"].tobytes()
    # not in place: the same arrays, nothing written
    ad2 = _adata(x, column)
    s2, n2 = cnv.tl.cnv_silhouette(ad2, inplace=False)
    assert s2.tobytes() == s.tobytes() and n2.tolist() == nearest.tolist()
    assert "cnv_silhouette" not in ad2.obs.columns and "cnv_silhouette" not in ad2.uns


# ---- edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
@pytest.mark.parametrize("g", [2, 3])
def test_cell_counts_at_the_tile_sizes(n, g):
    check(points(n, 6, n), random_codes(n, g, n + 1))


@pytest.mark.parametrize("n_chunks", [None, 1, 2, 3, 5])
def test_groups_that_straddle_tiles_and_chunks(n_chunks):
    """Groups of 1, 63, 64, 65, 130, 2 and 129 cells in scattered rows: 1 + 1 + 1 + 2 + 3 + 1 + 3 = 12 j-tiles; the chunks
    cut them at every place as n_chunks goes through 1, 2, 3, 5 and 12 (None at this size: a tile per chunk)."""
    sizes = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 2, 2, 2 * TILE + 1]
    codes = np.repeat(np.arange(len(sizes)), sizes)
    np.random.default_rng(8).shuffle(codes)
    x = points(codes.shape[0], 9, 9)
    got, want = check(x, codes, n_chunks=n_chunks)
    assert got["s"][codes == 0].tolist() == [0.0]  # the group of one cell


@pytest.mark.parametrize("c", [1, 2, 7, 8, 9, STAGE - 1, STAGE, STAGE + 1, 50, 2 * STAGE, 2 * STAGE + 1, 255, 256])
def test_component_counts_at_the_stage_sizes(c):
    check(points(70, c, c), random_codes(70, 3, c + 1, missing=0.05))
    check(_cuda(points(70, c, c, dtype=np.float64)), random_codes(70, 3, c + 1))


def test_more_than_64_groups():
    codes = random_codes(300, 70, 11, missing=0.05)
    check(points(300, 5, 10), codes, n_groups=70)
    check(points(300, 5, 10), codes, n_groups=70, n_chunks=4)


def test_every_group_a_pair():
    codes = np.repeat(np.arange(100), 2)
    np.random.default_rng(12).shuffle(codes)
    check(points(200, 4, 13), codes)
    check(points(200, 4, 13), codes, n_chunks=7)


def test_unused_groups_singletons_and_unlabelled_cells_interleaved():
    n = 140
    codes = np.tile([0, -1, 3, 3, 0, -1, 5], n // 7)  # groups 1, 2, 4 and 6 .. 8 have no cells
    codes[10] = 7                                      # ... and group 7 one
    got, want = check(points(n, 3, 14), codes, n_groups=9)
    assert np.isnan(got["s"][codes < 0]).all() and (got["nearest"][codes < 0] == -1).all()
    assert got["s"][10] == 0.0 and got["a"][10] == 0.0 and got["b"][10] > 0.0
    # the unlabelled cells are in no sum
    keep = codes >= 0
    sub = widths(points(n, 3, 14)[keep], codes[keep], 9)
    assert sub["s"].tobytes() == got["s"][keep].tobytes()


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def test_rounding_pin_is_ties_to_even():
    x = (np.arange(9) * 2.0 ** -41).reshape(9, 1)
    codes = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2])
    got, want = check(x, codes)
    assert want["S"][0].tolist() == [1, 9, 8] and got["shift"] == 40
    # a(0) = 1 / (2 2^40) and b(0) = 9 / (4 2^40), group 1 (group 2: 8 / (2 2^40)); half-up would give 2 / .. and 10 / ..
    assert got["a"][0] == 1.0 / (2.0 * 2.0 ** 40) and got["b"][0] == 9.0 / (4.0 * 2.0 ** 40)
    assert got["nearest"][0] == 1


def test_rounding_pin_without_the_addition_form():
    """The same ties where e + dist_exp > 51 (rint and a conversion): one far cell makes m 2^12, e stays 40."""
    x = np.concatenate([np.arange(9) * 2.0 ** -41, [4096.0, 4096.0]]).reshape(11, 1)
    codes = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3])
    got, want = check(x, codes)
    assert got["shift"] == 40 and so.shift_of(4096.0, 4, 1)[1] + 40 > 51
    assert want["S"][0].tolist()[:3] == [1, 9, 8]


def test_identical_points_have_width_zero_not_nan():
    x = np.full((130, 3), 1.25, dtype=np.float32)
    codes = random_codes(130, 3, 15)
    got, _ = check(x, codes)
    assert (got["s"] == 0.0).all() and (got["a"] == 0.0).all() and (got["b"] == 0.0).all()
    assert not np.signbit(got["s"]).any()
    check(np.zeros((70, 2)), random_codes(70, 2, 16))  # m == 0: e = 40


@pytest.mark.parametrize("scale", [2.0 ** 20, 2.0 ** 30, 2.0 ** 45])
def test_large_values_lower_the_shift(scale):
    x = points(130, 6, 17, scale=scale, dtype=np.float64)
    got, want = check(x, random_codes(130, 3, 18))
    assert got["shift"] < 40 and got["shift"] == want["shift"]


@pytest.mark.parametrize("m", [255.9, 256.0])
def test_both_sides_of_the_addition_forms_limit(m):
    """C = 7 gives hc = 2: below 256 dist_exp = 11 and e + dist_exp = 51 (the addition form), at 256 it is 52."""
    x = np.random.default_rng(19).uniform(-m, m, (100, 7))
    x[0], x[1] = m, -m  # the two farthest cells a distance can have
    _, want = check(x, random_codes(100, 3, 20))
    assert want["shift"] + so.shift_of(m, 100, 7)[1] == (51 if m < 256 else 52)


def test_sums_beyond_2_to_53():
    rng = np.random.default_rng(59)
    x, codes = rng.uniform(-2048.0, 2048.0, (130, 4)), np.repeat([0, 1], [66, 64])
    _, want = check(x, codes)
    assert int(want["S"].max()).bit_length() > 53 and want["shift"] == 40
    check(x, codes, n_chunks=1)


def test_a_row_permutation_permutes_the_bytes_and_changes_none():
    x, codes, want = storage_case()
    perm = np.random.default_rng(21).permutation(x.shape[0])
    got = widths(x[perm], codes[perm], 4)
    for name in ("s", "a", "b"):
        assert got[name].tobytes() == want[name][perm].tobytes()
    assert got["nearest"].tolist() == want["nearest"][perm].tolist()


@pytest.mark.parametrize("budget", [1, 8 * 5 * 2 * TILE, 8 * 5 * 3 * TILE + 8])
def test_row_slabs_of_the_table_change_no_byte(budget):
    """330 labelled cells in 5 groups: slabs of 64, 128 and 192 positions (6, 3 and 2 slabs, the last one partial)."""
    x, codes = points(330, 8, 22), random_codes(330, 5, 23)
    want = so.silhouette(x.astype(np.float64), codes, 5)
    same(widths(x, codes, 5, s_budget=budget), want)
    same(widths(x, codes, 5, s_budget=budget, n_chunks=2), want)


def test_stage_times_come_from_device_events():
    x, codes, want = storage_case()
    stage_ms = {}
    same(widths(x, codes, 4, stage_ms=stage_ms), want)
    assert set(stage_ms) == {"sums", "finish"} and all(v > 0 for v in stage_ms.values())


# ---- the planted clones, through the public function ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_planted_clones(seed):
    import infercnvpy_amd as cnv

    x, true = so.planted(seed)
    rng = np.random.default_rng(1000 + seed)
    merged = np.where(true == 2, 1, true)
    split = true.copy()
    split[rng.permutation(60)[:30]] = 3
    shuffled = rng.permutation(true)
    means = []
    for codes in (true, merged, split, shuffled):
        ad = _adata(x, [f"clone{c}" for c in codes])
        cnv.tl.cnv_silhouette(ad)
        want = so.silhouette(x.astype(np.float64), pd.factorize(np.asarray(ad.obs["cnv_leiden"]))[0])
        assert ad.obs["cnv_silhouette"].to_numpy().tobytes() == want["s"].tobytes()
        assert ad.uns["cnv_silhouette"]["mean"] == want["mean"]
        means.append(ad.uns["cnv_silhouette"]["mean"])
    assert means[0] > means[1] > means[2] > means[3] and means[3] < 0
    moved = true.copy()
    moved[[0, 12, 24, 36, 48]] = 1
    ad = _adata(x, pd.Categorical.from_codes(moved, categories=["c0", "c1", "c2"]))
    cnv.tl.cnv_silhouette(ad)
    at = [0, 12, 24, 36, 48]
    assert (ad.obs["cnv_silhouette"].to_numpy()[at] < 0).all()
    assert (ad.obs["cnv_silhouette_nearest"].to_numpy()[at] == "c0").all()


# ---- device errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_in_a_cuda_tensor_raises(bad):
    import infercnvpy_amd as cnv

    x, codes, _ = storage_case()
    x = x.copy()
    x[77, 3] = bad
    ad = _adata(_cuda(x), [str(c) for c in np.maximum(codes, 0)])
    with pytest.raises(ValueError, match="X_cnv_pca has non-finite values"):
        cnv.tl.cnv_silhouette(ad)
    assert "cnv_silhouette" not in ad.obs.columns


def test_the_kernel_flags_a_non_finite_value_it_reads():
    from infercnvpy_amd import _engine
    from infercnvpy_amd.tl._groups import group_table

    x, codes, _ = storage_case()
    rows, group_ptr, _ = group_table(codes, 4)
    for bad_row, expect in ((int(rows[5]), 1), (int(np.flatnonzero(codes < 0)[0]), 0)):  # (an unlabelled row is not read)
        y = x.copy()
        y[bad_row, 6] = np.nan
        flags = _engine.silhouette(_engine.matrix_input(y, "test"), rows, group_ptr, 40, 5)[4]
        assert int(flags.item()) & 1 == expect

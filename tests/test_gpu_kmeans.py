"""tl.cnv_kmeans on the GPU equals the oracle of DESIGN.md 4.27 (tests/_kmeans_oracle.py) byte for byte: labels, centres,
distances, the integer inertia, the history of every run and the seeded rows, for every storage of the representation,
the sizes at which a kernel takes another path (cell tiles, centre tiles, component stages, seeding blocks, update slabs)
and the arithmetic pins (ties to the lowest centre, ties to even, sums past float64's integers, reduced shifts)."""
import functools

import numpy as np
import pytest

import _kmeans_oracle as ko
from test_kmeans_oracle import ari

pytestmark = pytest.mark.gpu

TILE_CELLS, TILE_CENTRES, STAGE, SEED_ROWS, UPDATE_ROWS = 256, 16, 32, 256, 1024  # (asserted below)


def points(n, c, seed, scale=1.0, dtype=np.float32):
    return (np.random.default_rng(seed).normal(0.0, 1.0, (n, c)) * scale).astype(dtype)


def _adata(x):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv_pca"] = x
    return ad


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fit(x, k, **kw):
    """The public call: (adata, codes, centers, info)."""
    import infercnvpy_amd as cnv

    ad = _adata(x)
    codes, centers, info = cnv.tl.cnv_kmeans(ad, k, return_info=True, **kw)
    return ad, codes, centers, info


def same(got, want, k):
    """Everything the call returns and stores against the oracle's dict."""
    ad, codes, centers, info = got
    assert codes.dtype == np.int32 and codes.tolist() == want["labels"].tolist()
    assert centers.dtype == np.float64 and centers.tobytes() == want["centers"].tobytes()
    dist = ad.obs["cnv_kmeans_distance"].to_numpy()
    assert dist.dtype == np.float64 and dist.tobytes() == want["distance"].tobytes()
    assert ad.obs["cnv_kmeans"].cat.codes.tolist() == want["labels"].tolist()
    assert list(ad.obs["cnv_kmeans"].cat.categories) == [str(j) for j in range(k)]
    uns = ad.uns["cnv_kmeans"]
    assert uns["centers"].tobytes() == want["centers"].tobytes()
    assert uns["sizes"].tolist() == want["sizes"].tolist()
    assert uns["inertia"] == want["inertia"] and uns["shift"] == want["shift"]
    assert (uns["n_iter"], uns["converged"], uns["best_init"]) == (want["n_iter"], want["converged"], want["best_init"])
    assert info["inertia_q"] == want["inertia_all"] and info["inertia_q"][uns["best_init"]] == want["inertia_q"]
    assert [[tuple(step) for step in run] for run in info["history"]] == want["history"]
    assert info["picks"] == (want["picks"] if want["picks"][0] is not None else None)


def check(x, k, **kw):
    host = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    want = ko.kmeans(host.astype(np.float64), k, **{"n_init": 2, **kw})
    got = fit(x, k, **{"n_init": 2, **kw})
    same(got, want, k)
    return got, want


def test_tile_constants():
    from infercnvpy_amd import _lib

    assert (_lib.ICV_KMEANS_TILE_CELLS, _lib.ICV_KMEANS_TILE_CENTRES, _lib.ICV_KMEANS_TILE_C, _lib.ICV_KMEANS_SEED_ROWS,
            _lib.ICV_KMEANS_UPDATE_ROWS) == (TILE_CELLS, TILE_CENTRES, STAGE, SEED_ROWS, UPDATE_ROWS)


# ---- storage ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def storage_case():
    x = points(150, 7, 1)
    return x, ko.kmeans(x.astype(np.float64), 4, n_init=3)


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
    x, want = storage_case()
    stored = STORAGE[kind](x)
    if kind in ("host_view", "cuda_view"):
        assert not (stored.flags["C_CONTIGUOUS"] if isinstance(stored, np.ndarray) else stored.is_contiguous())
    same(fit(stored, 4, n_init=3), want, 4)


def test_float64_values_and_other_dtypes():
    x = np.random.default_rng(5).normal(0, 1, (90, 5))  # (float64 values that float32 cannot hold)
    check(x, 3)
    check(_cuda(x), 3)
    h = x.astype(np.float16)
    same(fit(h, 3, n_init=2), ko.kmeans(h.astype(np.float64), 3, n_init=2), 3)
    i = np.round(x * 10).astype(np.int32)
    same(fit(i, 3, n_init=2), ko.kmeans(i.astype(np.float64), 3, n_init=2), 3)


# ---- sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257])
def test_cell_tile_edges(n):
    x = points(n, 4, 10 + n)
    check(x, 2)
    if n > 2:
        check(x, min(n, 5))


def test_every_point_its_own_centre():
    x = points(7, 3, 3)
    (ad, codes, _, info), want = check(x, 7)
    assert sorted(codes.tolist()) == list(range(7)) and want["inertia_q"] == 0
    assert ad.obs["cnv_kmeans_distance"].tolist() == [0.0] * 7


@pytest.mark.parametrize("k", [2, 3, 15, 16, 17, 63, 64, 65, 256])
def test_centre_tile_edges_and_the_cap(k):
    x = points(600 if k == 256 else 300, 5, 20 + k)
    check(x, k, n_init=1 if k >= 63 else 2)


@pytest.mark.parametrize("c", [1, 2, 7, 8, 9, 31, 32, 33, 50, 64, 65, 255, 256])
def test_component_stage_edges_and_the_cap(c):
    check(points(70, c, 40 + c), 3)


def test_rows_over_several_seeding_blocks_and_update_slabs():
    n = UPDATE_ROWS + 76
    assert n > 4 * SEED_ROWS
    x = points(n, 3, 7)
    x[:, 0] += np.repeat([0.0, 4.0, 8.0, 12.0], n // 4)  # (the clusters are runs of rows: the draws land in several blocks)
    (_, _, _, info), _ = check(x, 4, n_init=3)
    assert len({p // SEED_ROWS for run in info["picks"] for p in run}) >= 3


# ---- ties to the lowest centre ------------------------------------------------------------------------------------------------
def test_equidistant_from_centres_0_and_2():
    init = np.array([[1.0, 0.0], [50.0, 0.0], [-1.0, 0.0], [0.0, 60.0]])
    x = np.array([[0.0, 0.0], [0.0, 0.5], [50.0, 1.0], [-1.0, 0.25], [0.0, 60.0], [1.0, 0.0]], dtype=np.float32)
    (ad, codes, centers, _), want = check(x, 4, init=init, max_iter=1)
    # rows 0 and 1 are as far from centre 0 as from centre 2 and go to centre 0, whose first coordinate is + 1
    assert centers[codes[0], 0] == 1.0 and centers[codes[1], 0] == 1.0 and centers[codes[3], 0] == -1.0


def test_equidistant_from_centres_in_two_centre_tiles():
    k = 2 * TILE_CENTRES + 3
    init = np.zeros((k, 1))
    init[:, 0] = 100.0 + 10.0 * np.arange(k)
    init[3, 0], init[TILE_CENTRES + 4, 0], init[2 * TILE_CENTRES + 1, 0] = 1.0, -1.0, -1.0
    x = np.concatenate([[0.0, 0.0, 0.25], init[:, 0]]).astype(np.float32)[:, None]
    (_, codes, centers, _), _ = check(x, k, init=init, max_iter=1)
    assert centers[codes[0], 0] == 1.0 and centers[codes[1], 0] == 1.0 and centers[codes[2], 0] == 1.0
    # the same with the lower index in the later position of the tie: centre 3 at -1, the later ones at +1
    init[3, 0], init[TILE_CENTRES + 4, 0], init[2 * TILE_CENTRES + 1, 0] = -1.0, 1.0, 1.0
    (_, codes, centers, _), _ = check(x, k, init=init, max_iter=1)
    assert centers[codes[0], 0] == -1.0 and centers[codes[1], 0] == -1.0 and centers[codes[2], 0] == 1.0


# ---- empty clusters and renumbering -------------------------------------------------------------------------------------------
def test_an_empty_cluster_keeps_its_centre_and_comes_last():
    x = np.array([[0.0], [0.1], [1.0], [1.1], [1.2]], dtype=np.float32)
    init = np.array([[100.0], [0.0], [1.0]])
    (ad, codes, centers, info), _ = check(x, 3, init=init)
    assert ad.uns["cnv_kmeans"]["sizes"].tolist() == [3, 2, 0] and centers[2, 0] == 100.0
    assert codes.tolist() == [1, 1, 0, 0, 0] and len(ad.obs["cnv_kmeans"].cat.categories) == 3
    assert info["picks"] is None and ad.uns["cnv_kmeans"]["params"]["init"] == "array"


def test_two_clusters_of_equal_size_keep_their_raw_order():
    x = np.array([[5.0], [5.5], [0.0], [0.5], [9.0]], dtype=np.float32)
    init = np.array([[9.0], [5.0], [0.0]])
    (ad, codes, centers, _), _ = check(x, 3, init=init)
    assert centers[:, 0].tolist() == [5.25, 0.25, 9.0] and codes.tolist() == [0, 0, 1, 1, 2]


# ---- rounding -----------------------------------------------------------------------------------------------------------------
def test_ties_to_even_in_the_coordinates():
    x = (np.arange(8, dtype=np.float64) * 2.0 ** -41)[:, None]
    (_, _, centers, _), _ = check(x, 2, init=np.array([[0.0], [1.0]]), max_iter=2)
    assert centers[0, 0] == 14.0 / (8.0 * 2.0 ** 40)


def test_ties_to_even_in_the_weights_and_the_inertia():
    y = np.zeros((4, 2))
    y[:, 0] = [2.0 ** -21, 2.0 ** -21, 2.0 ** -20, 2.0 ** -20]
    y[:, 1] = [2.0 ** -21, 0.0, 2.0 ** -21, 2.0 ** -20]  # D from the origin: 0.5, 0.25, 1.25 and 2 units of 2^-40
    (_, _, _, info), _ = check(y, 2, init=np.array([[0.0, 0.0], [1.0, 1.0]]), max_iter=1)
    assert info["inertia_q"] == [3]
    # the seeding weights: whichever row comes first, every w is D 2^40 rounded to even (the oracle's picks hold)
    z = np.concatenate([np.zeros((1, 2)), y])
    first = set()
    for seed in range(12):
        row = ko.mix(ko.run_base(seed, 0)) % 5
        first.add(row)
        if row == 1:  # from row 1 the squared distances are 0.5, 0.25, 0.25 and 0.5 units: every w rounds to 0
            with pytest.raises(ValueError, match="fewer than 2 distinct points"):
                fit(z, 2, random_state=seed, n_init=1)
            continue
        (_, _, _, info), _ = check(z, 2, random_state=seed, n_init=1)
        assert info["picks"][0][0] == row
        if row == 0:  # from the origin w = 0, 0, 0, 1, 2: rows 1 and 2 (half and a quarter) are never drawn
            assert info["picks"][0][1] in (3, 4)
    assert {0, 1} <= first


def test_sums_past_the_integers_of_float64():
    x = np.random.default_rng(11).uniform(-2.0 ** 11, 2.0 ** 11, (130, 4))
    x[0, 0] = 2.0 ** 11  # (the bound itself: b = 12)
    _, want = check(x, 2)
    assert want["shift"] == (40, 25)
    q = np.rint(x * 2.0 ** 40).astype(np.int64)
    assert max(abs(int(q[want["labels"] == g, c].sum())) for g in range(2) for c in range(4)) > 2 ** 53


def test_reduced_shifts_and_values_too_large():
    import infercnvpy_amd as cnv

    x, _ = ko.planted(0)
    big = x.astype(np.float64) * 2.0 ** 20
    _, want = check(big, 3)
    assert want["shift"][0] < 40 and 0 <= want["shift"][1] < 40
    for stored in (x.astype(np.float64) * 2.0 ** 28, _cuda(x.astype(np.float64) * 2.0 ** 28)):
        with pytest.raises(ValueError, match="rescale X_cnv_pca"):
            cnv.tl.cnv_kmeans(_adata(stored), 3)


def test_a_non_finite_value_on_the_device():
    import infercnvpy_amd as cnv

    x = points(40, 3, 1)
    x[17, 2] = np.nan
    with pytest.raises(ValueError, match="X_cnv_pca has non-finite values"):
        cnv.tl.cnv_kmeans(_adata(_cuda(x)), 2)


# ---- seeding ------------------------------------------------------------------------------------------------------------------
def test_the_five_point_draws():
    from test_kmeans_oracle import FIVE

    for seed in range(64):
        want = ko.kmeans(FIVE, 3, random_state=seed, n_init=1)
        got = fit(FIVE, 3, random_state=seed, n_init=1)
        assert got[3]["picks"] == want["picks"]
        if seed < 4:
            same(got, want, 3)


def test_the_draws_at_the_boundaries_of_the_prefix_sum():
    x = np.arange(8, dtype=np.float64)[:, None] * 2.0 ** -20  # (test_kmeans_oracle: theta falls on P_i and on P_i - 1)
    for seed in range(64):
        assert fit(x, 2, random_state=seed, n_init=1)[3]["picks"] == ko.kmeans(x, 2, random_state=seed, n_init=1)["picks"]


def test_duplicates():
    import infercnvpy_amd as cnv

    x = np.array([0.0] * 4 + [1.0] * 4 + [5.0] * 2)[:, None]
    (_, _, _, info), _ = check(x, 2, random_state=0)
    assert info["picks"][0] == [0, 8]
    (_, _, _, info), _ = check(x, 3, random_state=0)
    assert info["picks"][0] == [0, 8, 5]
    ad = _adata(x)
    with pytest.raises(ValueError, match="fewer than 4 distinct points"):
        cnv.tl.cnv_kmeans(ad, 4)
    assert "cnv_kmeans" not in ad.obs.columns and "cnv_kmeans" not in ad.uns


# ---- the loop and the restarts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 2])
def test_a_run_cut_short_is_consistent(max_iter):
    x, _ = ko.planted(0)
    (ad, codes, centers, info), want = check(x, 3, max_iter=max_iter, n_init=3)
    assert ad.uns["cnv_kmeans"]["converged"] is False and ad.uns["cnv_kmeans"]["n_iter"] == max_iter
    assert all(len(run) == max_iter for run in info["history"])
    assert codes.tolist() == np.argmin(ko.sqdist(x.astype(np.float64), centers), axis=1).tolist()


def test_the_lowest_run_wins_a_tie():
    x = np.array([[0.0], [1.0], [10.0], [11.0]], dtype=np.float32)
    (ad, _, _, info), _ = check(x, 2, n_init=4)
    assert len(set(info["inertia_q"])) == 1 and ad.uns["cnv_kmeans"]["best_init"] == 0


def test_the_prototypes_winning_run():
    x, _ = ko.planted(4)
    (ad, _, _, _), _ = check(x, 3, n_init=10)
    assert ad.uns["cnv_kmeans"]["best_init"] == 2 and ad.uns["cnv_kmeans"]["params"]["n_init"] == 10


def test_rows_permuted_under_a_given_init():
    x, _ = ko.planted(2)
    init = x[[0, 70, 110]].astype(np.float64) + 0.125
    perm = np.random.default_rng(0).permutation(x.shape[0])
    _, codes, centers, _ = fit(x, 3, init=init)
    _, codes_p, centers_p, _ = fit(x[perm], 3, init=init)
    assert codes_p.tolist() == codes[perm].tolist() and centers_p.tobytes() == centers.tobytes()


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_planted_clones_are_recovered(seed):
    x, true = ko.planted(seed)
    (ad, codes, _, _), want = check(x, 3, n_init=10)
    printed = {0: 292.6063, 1: 301.2957, 2: 301.2923, 3: 301.3834, 4: 318.9760}[seed]  # scikit-learn's inertia
    assert abs(ad.uns["cnv_kmeans"]["inertia"] - printed) < 1e-4
    assert ari(true, codes) >= 0.95


def test_the_silhouette_prefers_three_clones():
    import infercnvpy_amd as cnv

    x, _ = ko.planted(0)
    ad = _adata(x)
    mean = {}
    for k in (2, 3, 4):
        cnv.tl.cnv_kmeans(ad, k)
        cnv.tl.cnv_silhouette(ad, "cnv_kmeans")
        mean[k] = ad.uns["cnv_silhouette"]["mean"]
    assert mean[3] > mean[2] and mean[3] > mean[4]


def test_known_centres_assign_a_second_sample():
    x, _ = ko.planted(0)
    y, true = ko.planted(1)
    _, _, centers, _ = fit(x, 3)
    (ad, codes, centers_y, info), _ = check(y, 3, init=centers, max_iter=1)
    assert sorted(map(bytes, centers_y)) == sorted(map(bytes, centers))  # (the centres, in the order of the new sizes)
    assert codes.tolist() == np.argmin(ko.sqdist(y.astype(np.float64), centers_y), axis=1).tolist()
    assert len(info["history"]) == 1 and len(info["history"][0]) == 1 and ari(true, codes) >= 0.9


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_the_public_forms():
    import pandas as pd

    import infercnvpy_amd as cnv

    x, _ = ko.planted(3)
    want = ko.kmeans(x.astype(np.float64), 3, random_state=5, n_init=2)
    ad = _adata(x)
    assert cnv.tl.cnv_kmeans(ad, 3, random_state=5, n_init=2, key_added="clone") is None
    assert isinstance(ad.obs["clone"].dtype, pd.CategoricalDtype) and ad.obs["clone"].cat.codes.tolist() == want["labels"].tolist()
    assert ad.obs["clone_distance"].to_numpy().tobytes() == want["distance"].tobytes()
    assert set(ad.uns["clone"]) == {"params", "centers", "sizes", "inertia", "n_iter", "converged", "shift", "best_init"}
    assert ad.uns["clone"]["params"] == {"n_clusters": 3, "use_rep": "cnv_pca", "random_state": 5, "n_init": 2,
                                         "max_iter": 300, "init": "k-means++"}
    ad2 = _adata(x)
    ad2.obsm["X_other"] = ad2.obsm.pop("X_cnv_pca")
    codes, centers = cnv.tl.cnv_kmeans(ad2, 3, use_rep="other", random_state=5, n_init=2, inplace=False)
    assert codes.dtype == np.int32 and codes.tolist() == want["labels"].tolist() and centers.tobytes() == want["centers"].tobytes()
    assert not list(ad2.obs.columns) and not ad2.uns
    codes, centers, info = cnv.tl.cnv_kmeans(ad2, 3, use_rep="other", random_state=5, n_init=2, inplace=False, return_info=True)
    assert set(info) == {"history", "picks", "inertia_q", "stage_ms"} and not list(ad2.obs.columns) and not ad2.uns
    assert set(info["stage_ms"]) == {"seed", "lloyd", "kmeans"} and info["picks"] == want["picks"]

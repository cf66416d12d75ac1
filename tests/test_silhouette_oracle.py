"""The oracle of tl.cnv_silhouette (tests/_silhouette_oracle.py) against a brute force, scikit-learn, the
planted clones, the rounding pin and identical points.  No test here needs a device.

The tolerance against the brute force is derived: quantisation moves a distance by at most 2^-(e+1), so a mean by at
most 2^-(e+1); s = (b - a) / max(a, b) moves by at most 4 2^-(e+1) / max(a, b) to first order, and 1e-15 covers the
float64 roundings of both sides.
"""
import functools

import numpy as np
import pytest

import _silhouette_oracle as so


def case_59_bits():
    """130 x 4 uniform in +-2^11, groups of 66 and 64: e = 40 and sums beyond 2^53."""
    rng = np.random.default_rng(59)
    return rng.uniform(-2048.0, 2048.0, (130, 4)), np.repeat([0, 1], [66, 64])


def relabelled(true):
    """Cells 0, 12, 24, 36, 48 of clone 0 relabelled as clone 1."""
    codes = true.copy()
    codes[[0, 12, 24, 36, 48]] = 1
    return codes


@functools.lru_cache(maxsize=None)
def planted_means(seed):
    """(true, merged, split, shuffled) mean widths of the planted case."""
    x, true = so.planted(seed)
    rng = np.random.default_rng(1000 + seed)
    merged = np.where(true == 2, 1, true)
    split = true.copy()
    split[rng.permutation(60)[:30]] = 3
    shuffled = rng.permutation(true)
    return tuple(so.silhouette(x, codes)["mean"] for codes in (true, merged, split, shuffled))


@pytest.mark.parametrize("name", ["planted", "59_bits"])
def test_oracle_equals_the_brute_force_within_the_quantisation(name):
    x, codes = so.planted(0) if name == "planted" else case_59_bits()
    res = so.silhouette(x, codes)
    s, a, b = so.brute_force(x, codes)
    e = res["shift"]
    bound = 4 * 2.0 ** -(e + 1) / np.maximum(a, b).min() + 1e-15
    worst = np.abs(res["s"] - s).max()
    print(f"{name}: e = {e}, largest |ds| = {worst:.3g}, bound = {bound:.3g}, largest S has "
          f"{int(res['S'].max()).bit_length()} bits")
    assert worst <= bound
    assert np.abs(res["a"] - a).max() <= 2.0 ** -(e + 1) + 4e-16 * a.max()
    assert np.abs(res["b"] - b).max() <= 2.0 ** -(e + 1) + 4e-16 * b.max()


def test_the_59_bit_case_has_sums_beyond_2_to_53():
    x, codes = case_59_bits()
    res = so.silhouette(x, codes)
    assert res["shift"] == 40
    assert int(res["S"].max()).bit_length() > 53
    assert int(res["S"].max()) < 2 ** 62


def test_oracle_equals_sklearn_on_separated_points():
    metrics = pytest.importorskip("sklearn.metrics")
    for x, codes in (so.planted(0), case_59_bits()):
        x = np.asarray(x, dtype=np.float64)
        res = so.silhouette(x, codes)
        theirs = metrics.silhouette_samples(x, codes, metric="euclidean")
        # (sklearn forms the distances from the Gram matrix in float64: ~1e-7 relative on a distance at worst)
        assert np.abs(res["s"] - theirs).max() < 1e-6
        assert abs(res["mean"] - metrics.silhouette_score(x, codes)) < 1e-6


@pytest.mark.parametrize("seed", range(5))
def test_planted_clones_rank_the_labellings(seed):
    true, merged, split, shuffled = planted_means(seed)
    print(f"seed {seed}: true {true:.4f} merged {merged:.4f} split {split:.4f} shuffled {shuffled:.4f}")
    assert true > merged > split > shuffled
    assert shuffled < 0


@pytest.mark.parametrize("seed", range(5))
def test_planted_relabelled_cells_point_back_to_their_clone(seed):
    x, true = so.planted(seed)
    res = so.silhouette(x, relabelled(true))
    at = [0, 12, 24, 36, 48]
    assert (res["s"][at] < 0).all()
    assert (res["nearest"][at] == 0).all()


def test_rounding_pin_is_ties_to_even():
    x = (np.arange(9) * 2.0 ** -41).reshape(9, 1)
    codes = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2])
    res = so.silhouette(x, codes)
    assert res["shift"] == 40
    # d_0j 2^40 = j / 2: 0, .5, 1 | 1.5, 2, 2.5, 3 | 3.5, 4 -> ties to even 0 0 1 | 2 2 2 3 | 4 4; half-up gives [2, 10, 8]
    assert res["S"][0].tolist() == [1, 9, 8]


def test_identical_points_have_width_zero_not_nan():
    x = np.full((7, 3), 1.25, dtype=np.float32)
    res = so.silhouette(x, np.array([0, 0, 0, 1, 1, 2, 2]))
    assert (res["s"] == 0.0).all() and (res["a"] == 0.0).all() and (res["b"] == 0.0).all()
    assert res["nearest"].tolist() == [1, 1, 1, 0, 0, 0, 0]


def test_singleton_unlabelled_and_unused_groups():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (12, 5)).astype(np.float32)
    codes = np.array([0, 0, 0, 2, -1, 2, 2, 4, 0, -1, 2, 0])  # groups 1 and 3 unused, group 4 one cell
    res = so.silhouette(x, codes, n_groups=6)
    assert res["s"][7] == 0.0 and res["a"][7] == 0.0 and res["b"][7] > 0 and res["nearest"][7] in (0, 2)
    assert np.isnan(res["s"][[4, 9]]).all() and (res["nearest"][[4, 9]] == -1).all()
    assert np.isnan(res["group_mean"][[1, 3, 5]]).all() and res["sizes"].tolist() == [5, 0, 4, 0, 1, 0]
    # the unlabelled cells are in no sum: dropping them changes no bit of the others
    keep = codes >= 0
    sub = so.silhouette(x[keep], codes[keep], n_groups=6)
    assert sub["s"].tobytes() == res["s"][keep].tobytes() and sub["mean"] == res["mean"]


def test_shift_rule():
    assert so.shift_of(0.0, 10, 50) == (40, 4)
    assert so.shift_of(1.0, 1, 1) == (40, 2)                  # b = 1, hc = 0
    assert so.shift_of(2047.9, 66, 4) == (40, 13)             # 61 - 7 - 13 = 41
    assert so.shift_of(2.0 ** 20, 1000, 256)[0] == 61 - 10 - (21 + 1 + 4)
    assert so.shift_of(2.0 ** 60, 2, 2)[0] < 0
    with pytest.raises(ValueError, match="e < 0"):
        so.silhouette(np.array([[2.0 ** 60], [0.0], [1.0], [2.0]]), np.array([0, 0, 1, 1]))
    with pytest.raises(ValueError, match="two non-empty"):
        so.silhouette(np.zeros((3, 2)), np.array([1, 1, -1]))

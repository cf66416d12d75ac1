"""The numpy oracle of tl.cnv_kmeans (tests/_kmeans_oracle.py) against scikit-learn, its own loop invariants, a big-int
restatement of the seeding draw and hand-computed ties.  No test here needs a device."""
import numpy as np
import pytest

import _kmeans_oracle as ko

PLANTED_SEEDS = (0, 1, 2, 3, 4)


def ari(a, b):
    """The adjusted Rand index of two labelings."""
    a, b = np.asarray(a), np.asarray(b)
    table = np.zeros((a.max() + 1, b.max() + 1), dtype=np.int64)
    np.add.at(table, (a, b), 1)
    pairs = lambda v: (v * (v - 1) // 2).sum()  # noqa: E731
    both, rows, cols, total = pairs(table), pairs(table.sum(axis=1)), pairs(table.sum(axis=0)), pairs(np.int64(a.shape[0]))
    expected = rows * cols / total
    return float((both - expected) / ((rows + cols) / 2 - expected))


@pytest.fixture(scope="module")
def cases():
    """name -> (x, truth, k, the oracle's result), computed once and left unchanged."""
    out = {}
    for seed in PLANTED_SEEDS:
        x, true = ko.planted(seed)
        out[f"planted{seed}"] = (x, true, 3, ko.kmeans(x, 3, random_state=0, n_init=10))
    x, true = ko.blobs(1)
    out["blobs1"] = (x, true, 8, ko.kmeans(x, 8, random_state=0, n_init=10))
    return out


NAMES = [f"planted{s}" for s in PLANTED_SEEDS] + ["blobs1"]


@pytest.mark.parametrize("name", NAMES)
def test_inertia_reaches_sklearns(cases, name):
    cluster = pytest.importorskip("sklearn.cluster")
    x, _, k, res = cases[name]
    ref = cluster.KMeans(n_clusters=k, n_init=10, random_state=0).fit(x.astype(np.float64))
    print(name, "oracle", res["inertia"], "sklearn", ref.inertia_)
    assert res["inertia"] <= ref.inertia_ * (1 + 1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_truth_is_recovered(cases, name):
    _, true, _, res = cases[name]
    score = ari(true, res["labels"])
    print(name, "ARI", score)
    if name == "blobs1":
        assert score == 1.0
    else:
        assert score >= 0.95


@pytest.mark.parametrize("name", NAMES)
def test_integer_inertia_never_rises_and_labels_are_the_argmin(cases, name):
    x, _, k, res = cases[name]
    for trace in res["history"]:
        inertia = [step[0] for step in trace]
        assert all(b <= a for a, b in zip(inertia, inertia[1:]))
        assert trace[0][1] == x.shape[0] and trace[-1][1] == 0
    assert res["converged"] and res["inertia_q"] == min(res["inertia_all"])
    assert res["best_init"] == res["inertia_all"].index(res["inertia_q"])
    d = ko.sqdist(x.astype(np.float64), res["centers"])
    assert np.array_equal(res["labels"], np.argmin(d, axis=1))
    assert np.array_equal(res["sqdist"], d.min(axis=1))
    assert np.array_equal(res["sizes"], np.bincount(res["labels"], minlength=k))
    assert (np.diff(res["sizes"]) <= 0).all()


def test_the_prototypes_winning_run():
    x, _ = ko.planted(4)
    assert ko.kmeans(x, 3, random_state=0, n_init=10)["best_init"] == 2


# ---- the seeding draw -----------------------------------------------------------------------------------------------------------
FIVE = np.array([[0.0], [1.0], [1.0], [3.0], [7.0]])  # from centre row 0: D = 0, 1, 1, 9, 49, w = D 2^f, P = 0, 1, 2, 11, 60 (2^f)


def _big_int_pick(w, z):
    """The first i with P_i > z mod W, in Python integers."""
    theta = z % sum(w)
    run = 0
    for i, wi in enumerate(w):
        run += wi
        if run > theta:
            return i
    raise AssertionError


def test_seeding_picks_equal_a_big_int_restatement():
    e, f = ko.shifts(7.0, 5, 1)
    assert (e, f) == (40, 40)
    on_p, below_p = 0, 0
    for seed in range(64):
        base = ko.run_base(seed, 0)
        picks = ko.seed_rows(FIVE, 3, f, base)
        first = ko.mix(base) % 5
        assert picks[0] == first
        d = (FIVE[:, 0] - FIVE[first, 0]) ** 2
        w = [int(v) << f for v in d]  # hand-computed: whole numbers times 2^f
        assert picks[1] == _big_int_pick(w, ko.mix(base ^ 1))
        d = np.minimum(d, (FIVE[:, 0] - FIVE[picks[1], 0]) ** 2)
        w2 = [int(v) << f for v in d]
        assert picks[2] == _big_int_pick(w2, ko.mix(base ^ 2))
        assert len(set(FIVE[picks, 0])) == 3


def test_seeding_at_the_boundaries_of_the_prefix_sum():
    """theta exactly on a P_i goes to the next row with weight; theta = P_i - 1 stays on row i.  The draw is made to
    fall there by choosing the weights: with w = (a, 0, c), theta = z mod (a + c) and a = theta or theta + 1."""
    z = ko.mix(ko.run_base(0, 0) ^ 1)
    for total in (1000, 12345, 2 ** 40 + 7):
        theta = z % total
        for a, want in ((theta, 2), (theta + 1, 0)):  # P_0 = theta: not > theta; P_0 - 1 = theta: row 0
            w = np.array([a, 0, total - a], dtype=np.int64)
            p = np.cumsum(w)
            assert int(np.searchsorted(p, z % int(p[-1]), side="right")) == want == _big_int_pick(w.tolist(), z)


def test_seeding_hits_both_boundaries_among_the_64_seeds():
    """Among seeds 0 .. 63 on the 8-point case below, theta falls exactly on a P_i and on a P_i - 1 (unit weights make
    every theta one of the two): the pick is the next row in the first case and the row itself in the second."""
    x = np.arange(8, dtype=np.float64)[:, None] * 2.0 ** -20  # D 2^f = (i - j)^2: whole numbers
    e, f = ko.shifts(float(x.max()), 8, 1)
    assert f == 40
    seen = set()
    for seed in range(64):
        base = ko.run_base(seed, 0)
        picks = ko.seed_rows(x, 2, f, base)
        w = [(i - picks[0]) ** 2 for i in range(8)]
        theta = ko.mix(base ^ 1) % sum(w)
        p = np.cumsum(w).tolist()
        assert picks[1] == _big_int_pick(w, ko.mix(base ^ 1))
        if theta in p:
            seen.add("on")
            assert picks[1] > p.index(theta)
        if theta + 1 in p:
            seen.add("below")
            assert picks[1] == p.index(theta + 1)
    assert seen == {"on", "below"}


def test_duplicates():
    x = np.array([0.0] * 4 + [1.0] * 4 + [5.0] * 2)[:, None]
    r2, r3 = ko.kmeans(x, 2, random_state=0), ko.kmeans(x, 3, random_state=0)
    assert r2["picks"][0] == [0, 8] and r3["picks"][0] == [0, 8, 5]
    assert r3["inertia_q"] == 0 and sorted(r3["centers"][:, 0].tolist()) == [0.0, 1.0, 5.0]
    assert r3["sizes"].tolist() == [4, 4, 2] and r3["centers"][:, 0].tolist()[2] == 5.0
    with pytest.raises(ValueError, match="fewer than 4 distinct points"):
        ko.kmeans(x, 4, random_state=0)


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def test_ties_to_even_in_q_and_w():
    # coordinates j 2^-41 with e = 40: q = rint(j / 2) to even
    x = (np.arange(8, dtype=np.float64) * 2.0 ** -41)[:, None]
    e, f = ko.shifts(float(x.max()), 8, 1)
    assert (e, f) == (40, 40)
    init = np.array([[0.0], [1.0]])
    res = ko.kmeans(x, 2, init=init, max_iter=2)
    # all cells go to centre 0; Q = sum of rint(j / 2) to even = 0 + 0 + 1 + 2 + 2 + 2 + 3 + 4 = 14
    assert res["history"][0][0][1] == 8 and res["sizes"].tolist() == [8, 0]
    assert res["centers"][0, 0] == 14.0 / (8.0 * 2.0 ** 40) and res["centers"][1, 0] == 1.0
    # squared distances j 2^-41 from centre 0 (x = sqrt of it is not exact, so give D by two components instead)
    y = np.zeros((4, 2))
    y[:, 0] = [2.0 ** -21, 2.0 ** -21, 2.0 ** -20, 2.0 ** -20]  # squares 2^-42, 2^-40
    y[:, 1] = [2.0 ** -21, 0.0, 2.0 ** -21, 2.0 ** -20]          # D = 2^-41, 2^-42, 5 2^-42, 2^-39
    far = np.array([[0.0, 0.0], [1.0, 1.0]])
    res = ko.kmeans(y, 2, init=far, max_iter=1)
    assert ko.shifts(1.0, 4, 2) == (40, 40)
    # rint(0.5) + rint(0.25) + rint(1.25) + rint(2) = 0 + 0 + 1 + 2
    assert res["inertia_q"] == 3 and res["history"][0] == [(3, 4)]


def test_a_point_between_two_centres_goes_to_the_lower_index():
    x = np.array([[0.0], [2.0], [1.0], [1.0]])
    res = ko.lloyd(x, np.array([[0.0], [2.0]]), 40, 40, 1)
    assert res[0].tolist() == [0, 1, 0, 0]
    res = ko.lloyd(x, np.array([[2.0], [0.0]]), 40, 40, 1)
    assert res[0].tolist() == [1, 0, 0, 0]


def test_shifts():
    assert ko.shifts(100, 10 ** 6, 50) == (35, 19)
    assert ko.shifts(2 ** 11, 130, 4) == (40, 25)
    assert ko.shifts(2 ** 30, 1000, 256)[1] < 0
    assert ko.shifts(0.0, 5, 3) == (40, 40)
    with pytest.raises(ValueError, match="rescale"):
        ko.kmeans(np.full((1000, 256), 2.0 ** 30), 2)


def test_an_empty_cluster_keeps_its_centre_and_comes_last():
    x = np.array([[0.0], [0.1], [1.0], [1.1], [1.2]])
    init = np.array([[100.0], [0.0], [1.0]])
    res = ko.kmeans(x, 3, init=init)
    assert res["sizes"].tolist() == [3, 2, 0] and res["centers"][2, 0] == 100.0
    assert res["labels"].tolist() == [1, 1, 0, 0, 0] and res["picks"] == [None]

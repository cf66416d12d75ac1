"""The numpy oracle of the Ward rounds (tests/_ward_oracle.py) checked on the CPU: against scipy on well-separated
data, against values worked out by hand, for the properties of a linkage, and for the tie paths its inputs reach.
tests/test_gpu_ward_exact.py then holds the kernels to this oracle bit for bit."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import is_valid_linkage, linkage
from scipy.spatial.distance import squareform

import _ward_cases as W
from _ward_oracle import leaf_hashes, leaf_sets, lw, ward_rounds
from test_gpu_parity import _blobs

BLOB_SHAPES = [(2, 4, 1), (3, 2, 1), (10, 3, 2), (257, 20, 6), (1000, 50, 8), (3000, 300, 12)]  # test_ward_linkage_matches_scipy's


def _sqdist32(X):
    x = X.astype(np.float64)
    g = x @ x.T
    D = np.triu(np.maximum(np.diag(g)[:, None] + np.diag(g)[None, :] - 2 * g, 0), 1).astype(np.float32)
    return D + D.T


def _check_linkage(Z, n):
    assert Z.shape == (n - 1, 4)
    if n > 2:
        assert is_valid_linkage(Z)
    assert np.all(np.diff(Z[:, 2]) >= 0) and Z[-1, 3] == n
    ids = np.concatenate([Z[:, 0], Z[:, 1]]).astype(np.int64)
    np.testing.assert_array_equal(np.sort(ids), np.arange(2 * n - 2))  # every id used exactly once
    assert np.all(Z[:, 0] < Z[:, 1])


@pytest.mark.parametrize("n,d,k", BLOB_SHAPES)
def test_oracle_matches_scipy_on_separated_data(n, d, k):
    D = _sqdist32(_blobs(n, d, k, seed=100 + n))
    Z, rounds = ward_rounds(D)
    Zs = linkage(squareform(np.sqrt(D.astype(np.float64)), checks=False), "ward")
    _check_linkage(Z, n)
    assert 1 <= rounds <= n - 1
    np.testing.assert_allclose(Z[:, 2], Zs[:, 2], rtol=1e-4)  # the project's bar against scipy
    assert leaf_hashes(Z) == leaf_hashes(Zs)  # the same leaf set for every merge
    np.testing.assert_array_equal(np.sort(Z[:, 3]), np.sort(Zs[:, 3]))


def test_two_and_three_points():
    Z, rounds = ward_rounds(np.array([[0, 9], [9, 0]], dtype=np.float32))
    np.testing.assert_array_equal(Z, [[0, 1, 3, 2]])
    assert rounds == 1
    # 0, 1, 3 on a line: (0, 1) at 1, then d2 = (2 * 9 + 2 * 4 - 1 * 1) / 3 = 25 / 3, rounded to float32
    D = np.array([[0, 1, 9], [1, 0, 4], [9, 4, 0]], dtype=np.float32)
    Z, rounds = ward_rounds(D)
    np.testing.assert_array_equal(Z, [[0, 1, 1, 2], [2, 3, np.sqrt(np.float64(np.float32(25 / 3))), 3]])
    assert rounds == 2
    assert ward_rounds(np.zeros((1, 1), dtype=np.float32))[0].shape == (0, 4)


def test_four_points_on_a_line():
    """0, 1, 10, 11: both pairs merge in round 0; the entry between them goes through the lower slot's merge first:
    xk = (2 * 100 + 2 * 81 - 1) / 3 (rounded to float32), xl = (2 * 121 + 2 * 100 - 1) / 3 = 147, then
    (3 xk + 3 xl - 2 * 1) / 4 -- 200 in exact arithmetic (centroids 10 apart, 2 * 2 * 2 / 4 * 100)."""
    p = np.array([0, 1, 10, 11], dtype=np.float64)
    D = ((p[:, None] - p[None, :]) ** 2).astype(np.float32)
    xk = float(np.float32((2.0 * 100.0 + 2.0 * 81.0 - 1.0) / 3.0))
    v = np.float32((3.0 * xk + 3.0 * 147.0 - 2.0 * 1.0) / 4.0)
    assert abs(float(v) - 200.0) < 1e-4
    Z, rounds = ward_rounds(D)
    np.testing.assert_array_equal(Z, [[0, 1, 1, 2], [2, 3, 1, 2], [4, 5, np.sqrt(np.float64(v)), 4]])
    assert rounds == 2
    # a swapped size in the first step gives another float32: the case can tell
    assert lw(np.float32(100), np.float32(81), np.float32(1), 1, 1, 1) == np.float32(xk)


def test_all_equal_matrix_merges_by_lowest_slot():
    """Every distance 1: all updates give 1 again ((2 + 2 - 1) / 3, (3 + 2 - 1) / 4, ...).  By the lowest-slot rule
    slot 0 points at slot 1 and every other slot at slot 0, so each round has the one pair (0, lowest other slot):
    a chain of n - 1 rounds, every parent at the height of its child, kept in log order by the stable sort."""
    stats = {}
    Z, rounds = ward_rounds(W.all_equal(5), stats)
    np.testing.assert_array_equal(Z, [[0, 1, 1, 2], [2, 5, 1, 3], [3, 6, 1, 4], [4, 7, 1, 5]])
    assert rounds == 4 and stats == {"pairless_passes": 0, "parent_at_child_height": 3}
    # two values: 0-1 and 2-3 are close, everything else far and equal -> both pairs in round 0, (0, 2) in round 1
    D = W.all_equal(4, 4.0)
    D[0, 1] = D[1, 0] = D[2, 3] = D[3, 2] = 1.0
    Z, rounds = ward_rounds(D)
    np.testing.assert_array_equal(Z[:2], [[0, 1, 1, 2], [2, 3, 1, 2]])
    np.testing.assert_array_equal(Z[2, [0, 1, 3]], [4, 5, 4])
    assert rounds == 2


def test_duplicates_at_distance_zero():
    """0, 0, 0, 5 on a line: (0, 1) at 0; slot 2's cached neighbour merged, it finds the new cluster at 0 again;
    slot 3 finds slot 2 at 25 (the cluster is at 100 / 3); (0, 2) at 0; then ((2 + 1) * 100 / 3 + (1 + 1) * 25) / 4."""
    p = np.array([0, 0, 0, 5], dtype=np.float64)
    D = ((p[:, None] - p[None, :]) ** 2).astype(np.float32)
    stats = {}
    Z, rounds = ward_rounds(D, stats)
    v = np.float32((3.0 * float(np.float32(100.0 / 3.0)) + 2.0 * 25.0 - 0.0) / 4.0)
    np.testing.assert_array_equal(Z, [[0, 1, 0, 2], [2, 4, 0, 3], [3, 5, np.sqrt(np.float64(v)), 4]])
    assert rounds == 3 and stats["parent_at_child_height"] == 1


@pytest.mark.parametrize("kind", W.TIE_KINDS)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 63, 64, 65, 257])
def test_properties_on_tied_matrices(kind, n):
    D = W.tie_matrix(kind, n)
    keep = D.copy()
    Z, rounds = ward_rounds(D)
    np.testing.assert_array_equal(D, keep)  # the input is not written
    _check_linkage(Z, n)
    assert 1 <= rounds <= n - 1
    Z2, rounds2 = ward_rounds(np.array(D, order="F"))
    np.testing.assert_array_equal(Z, Z2)
    assert rounds == rounds2
    assert [len(s) for s in leaf_sets(Z)] == Z[:, 3].astype(int).tolist()


def test_non_finite_distances_are_an_error():
    with pytest.raises(ValueError, match="not finite"):
        ward_rounds(W.all_equal(6, np.inf))
    D = W.all_equal(5)
    D[4, :4] = D[:4, 4] = np.inf  # a cluster nobody can reach: the others merge, then no pair is left
    with pytest.raises(ValueError, match="not finite"):
        ward_rounds(D)


def test_committed_cases_reach_the_tie_paths():
    """What tests/test_gpu_ward_exact.py runs on the GPU includes merges whose parent sits at the height of its
    child, at zero and at positive heights.  (The pass that searches every row again after a round without a pair
    was not reached by a seeded search over grids, two- and three-valued and small integer matrices: DESIGN.md
    section 5.)"""
    tied = {}
    for kind in W.TIE_KINDS:
        stats = {}
        Z, _ = ward_rounds(W.tie_matrix(kind, 65), stats)
        tied[kind] = stats["parent_at_child_height"]
    assert tied["equal"] > 0 and tied["int"] > 0 and tied["three"] > 0
    Z, _ = ward_rounds(W.tie_matrix("int", 65))
    assert (Z[:, 2] == 0).sum() >= 2  # duplicates

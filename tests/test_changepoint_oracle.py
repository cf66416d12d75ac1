"""The oracle of tl.cnv_changepoints (tests/_changepoint_oracle.py) against a brute force over all
segmentations, its scalar against its vectorised form, its fixed behaviours, the lane model of the kernel with the mutants
that each limit case tells apart, the planted case, and everything the function and its two entry points refuse before they
touch the device.  No GPU."""
import ctypes
import functools
import itertools
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _changepoint_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle against all segmentations --------------------------------------------------------------------------------------
def _brute_force(xs, beta, m):
    """The smallest total cost over every segmentation whose segments have at least m windows (the whole chromosome as
    one segment always counts), each segment's cost as numpy's sum of squared deviations from its mean."""
    L = len(xs)
    xs = np.asarray(xs, dtype=np.float64)
    best = math.inf
    for k in range(L):
        for cuts in itertools.combinations(range(1, L), k):
            edges = (0,) + cuts + (L,)
            if k and min(b - a for a, b in zip(edges, edges[1:])) < m:
                continue
            total = sum(float(((xs[a:b] - xs[a:b].mean()) ** 2).sum()) + beta for a, b in zip(edges, edges[1:]))
            best = min(best, total)
    return best


def test_the_oracle_finds_the_cheapest_of_all_segmentations():
    """216 random cases: L <= 11, m in {1, 2, 3}, beta in {0, 0.05, 0.3, 1}.  The costs are compared, not the
    segmentations (the brute force sums differently): the oracle's F_L is a sum of at most L costs, each with a forward
    error of a few L 2^-53 of values below 10, so 1e-9 is far above both sides' rounding."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for case in range(216):
        L = int(rng.integers(1, 12))
        m = (1, 2, 3)[case % 3]
        beta = (0.0, 0.05, 0.3, 1.0)[(case // 3) % 4]
        xs = rng.normal(0.0, 0.3, L) + rng.choice([0.0, 0.5, -0.5], L) * (rng.random() < 0.7)
        for vectorised in (False, True):
            _, _, segs, cost = co.segment_chromosome(xs, beta, m, vectorised)
            assert segs[0][0] == 0 and segs[-1][1] == L and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
            assert len(segs) == 1 or min(j - i for i, j in segs) >= m
            worst = max(worst, abs(cost - _brute_force(xs, beta, m)))
    print(f"largest |F_L - brute force| = {worst:.3g}")
    assert worst <= 1e-9


# ---- scalar against vectorised -------------------------------------------------------------------------------------------------
def test_the_scalar_and_the_vectorised_form_give_the_same_bytes():
    rng = np.random.default_rng(1)
    rows = [[-0.0, 1.22, 1.36]] + [rng.normal(0.0, 0.4, int(rng.integers(1, 40))).tolist() for _ in range(60)]
    rows += [(rng.integers(-3, 4, 24) * 0.25).tolist() for _ in range(20)]
    for k, xs in enumerate(rows):
        for m in (1, 2, 5):
            for beta in (0.0, 0.07, 0.5):
                a = co.segment_chromosome(xs, beta, m, False)
                b = co.segment_chromosome(xs, beta, m, True)
                assert a[2] == b[2], (k, m, beta)
                assert np.asarray(a[0]).tobytes() == np.asarray(b[0]).tobytes() and a[1] == b[1], (k, m, beta)
                assert a[3] == b[3] or (math.isinf(a[3]) and math.isinf(b[3]))


def test_the_chains_start_at_plus_zero():
    P, Q = co.prefix_chains([-0.0, 1.22, 1.36])
    assert P[0] == 0.0 and not math.copysign(1.0, P[1]) < 0 and P[1:] == [0.0, 1.22, 1.22 + 1.36]
    assert math.copysign(1.0, float(np.cumsum([-0.0, 1.22])[0])) < 0  # (what the written chain is not)
    levels, _, _, _ = co.segment_chromosome([-0.0, -0.0], 0.0, 1)
    assert np.asarray(levels).tobytes() == np.zeros(2).tobytes()


# ---- fixed behaviours ----------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_i():
    # a constant row under beta = 0: every segmentation costs 0.0, so every j takes i = 0
    for vectorised in (False, True):
        levels, starts, segs, cost = co.segment_chromosome([0.75] * 9, 0.0, 1, vectorised)
        assert segs == [(0, 9)] and starts == [1] + [0] * 8 and levels == [0.75] * 9 and cost == 0.0
        # multiples of 1/4: (0, 0, 1, 1) as one piece costs 1.0 + beta, as the pieces (0, 2] + (2, 4] 2 beta; at beta = 1
        # both cost 2.0, and F_4 takes the lower i = 0
        _, _, segs, cost = co.segment_chromosome([0.0, 0.0, 1.0, 1.0], 1.0, 1, vectorised)
        assert cost == 2.0 and segs == [(0, 4)]
        _, _, segs, cost = co.segment_chromosome([0.0, 0.0, 1.0, 1.0], 0.25, 1, vectorised)
        assert cost == 0.5 and segs == [(0, 2), (2, 4)]
        # 0.25, 0.75, 0.25 under beta = 0: the cuts after 1 and after 2 are both free once every window is its own piece
        _, starts, segs, cost = co.segment_chromosome([0.25, 0.75, 0.25], 0.0, 1, vectorised)
        assert cost == 0.0 and segs == [(0, 1), (1, 2), (2, 3)]
        # 1/4, 1/4, 3/4, 3/4, 1/4, 1/4 with m = 2 and beta = 1/8: three pieces cost 3/8; two pieces cost at least 1/4 +
        # 1/6 and one piece 1/3 + 1/8 -- and (0, 2] before (2, 4] is the only order
        _, _, segs, _ = co.segment_chromosome([0.25, 0.25, 0.75, 0.75, 0.25, 0.25], 0.125, 2, vectorised)
        assert segs == [(0, 2), (2, 4), (4, 6)]


def test_short_chromosomes_and_long_minimum_lengths():
    for vectorised in (False, True):
        assert co.segment_chromosome([0.4], 0.3, 1, vectorised)[:3] == ([0.4], [1], [(0, 1)])  # L = 1
        assert co.segment_chromosome([0.4], 0.3, 7, vectorised)[2] == [(0, 1)]
        xs = [0.0, 0.0, 5.0, 5.0, 5.0]
        assert co.segment_chromosome(xs, 0.0, 1, vectorised)[2] == [(0, 2), (2, 5)]
        assert co.segment_chromosome(xs, 0.0, 2, vectorised)[2] == [(0, 2), (2, 5)]
        assert co.segment_chromosome(xs, 0.0, 3, vectorised)[2] == [(0, 5)]  # (2, 5] has 3 windows, (0, 2] only 2
        assert co.segment_chromosome(xs, 0.0, 5, vectorised)[2] == [(0, 5)]  # L = m
        levels, starts, segs, cost = co.segment_chromosome(xs, 0.0, 6, vectorised)  # L < m
        assert segs == [(0, 5)] and starts == [1, 0, 0, 0, 0] and levels == [3.0] * 5 and cost == 30.0
        F, back, _ = (co.partition_vectorised if vectorised else co.partition)(xs, 0.0, 3)
        assert F[1] == F[2] == math.inf and F[3] < math.inf and back[5] == 0


def test_storage_and_stored_zeros_change_no_byte():
    rng = np.random.default_rng(4)
    dense = rng.normal(0.0, 0.5, (7, 60)) * (rng.random((7, 60)) < 0.3)
    dense[:, 0] = 0.0
    chr_pos = {"a": 0, "b": 25, "c": 26}
    want = co.cnv_changepoints(dense, chr_pos)
    csr = sp.csr_matrix(dense)
    filler = np.where(np.arange(dense.size) % 2 == 0, -0.0, 0.0).reshape(dense.shape)  # every entry stored: -0.0 and 0.0
    zeros = sp.csr_matrix((np.where(dense == 0, filler, dense).ravel(), np.tile(np.arange(60), 7), np.arange(8) * 60),
                          shape=(7, 60))
    assert zeros.nnz == 7 * 60 and np.signbit(zeros.data[zeros.data == 0]).any() and (zeros.toarray() == dense).all()
    assert math.copysign(1.0, co.rows_of(zeros)[0][0]) < 0  # the oracle sees the stored -0.0 at the head of the row
    for name, x in {"csr": csr, "csc": csr.tocsc(), "fortran": np.asfortranarray(dense), "stored_zeros": zeros,
                    "dense_minus_zero": np.where(dense == 0, filler, dense)}.items():
        got = co.cnv_changepoints(x, chr_pos)
        assert got["sigma"] == want["sigma"] and got["beta"] == want["beta"], name
        assert co.same_bytes(got["levels"], want["levels"]) and co.same_bytes(got["starts"], want["starts"]), name
        assert got["table"] == want["table"], name
    x32 = csr.astype(np.float32)
    assert co.same_bytes(co.cnv_changepoints(x32, chr_pos)["levels"],
                         co.cnv_changepoints(dense.astype(np.float32).astype(np.float64), chr_pos)["levels"])


def test_host_scalars():
    x = np.asarray([[0.0, 1.0, 3.0, 3.0, 7.0], [1.0, 1.0, 1.0, 2.0, 2.0]])
    chr_pos = {"a": 0, "b": 3}
    assert co.diffsq(co.rows_of(x), [0, 3, 5]) == [1.0 + 4.0 + 16.0, 0.0]  # no difference across the boundary 2 | 3
    assert co.default_sigma(x, chr_pos) == math.sqrt(21.0 / (2.0 * 6.0))  # M = 2 (5 - 2)
    assert co.default_sigma(np.ones((3, 2)), {"a": 0, "b": 1}) == 0.0  # M = 0
    got = co.cnv_changepoints(np.ones((3, 2)), {"a": 0, "b": 1})
    assert got["sigma"] == 0.0 and got["beta"] == 0.0 and got["n_segments"].tolist() == [2, 2, 2]
    assert co.penalty_of(2.0, 0.1, 270) == (2.0 * (0.1 * 0.1)) * math.log(270)
    assert co.penalty_of(2.0, 0.1, 1) == 0.0
    from infercnvpy_amd.tl._changepoints import default_sigma

    assert default_sigma([21.0, 0.0], 2, 5, 2) == co.default_sigma(x, chr_pos) and default_sigma([], 3, 2, 2) == 0.0
    assert default_sigma([1e308, 1e308], 2, 5, 2) == math.inf


def test_values_that_could_overflow_are_refused():
    chr_pos = {"a": 0}
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            co.cnv_changepoints(np.asarray([[0.0, bad, 1.0]]), chr_pos, sigma=0.1)
    with pytest.raises(ValueError, match="magnitude 1e\\+154"):
        co.cnv_changepoints(np.asarray([[0.0, 1e154, 1.0]]), chr_pos, sigma=0.1)
    with pytest.raises(ValueError, match="beta"):
        co.cnv_changepoints(np.asarray([[0.0, 1.0, 1.0]]), chr_pos, sigma=1e150, penalty=1e10)
    assert co.cnv_changepoints(np.asarray([[0.0, 1e150, 1.0]]), chr_pos, sigma=0.1)["n_segments"].tolist() == [3]


# ---- the lane model of the kernel, its mutants, and what each limit case tells apart ----------------------------------------------
def _chromosomes(name):
    """[(row number, chromosome number, its values as Python floats)] of a named case."""
    c = co.expected(name)
    edges = co.bounds(c["chr_pos"], c["x"].shape[1])
    return [(r, k, row[s0:s1]) for r, row in enumerate(co.rows_of(c["x"]))
            for k, (s0, s1) in enumerate(zip(edges[:-1], edges[1:]))]


@pytest.mark.parametrize("name", co.EDGE_CASES)
def test_the_lane_model_is_the_oracle_on_every_chromosome_of_the_limit_cases(name):
    c = co.expected(name)
    beta, m = c["want"]["beta"], c["kwargs"].get("min_windows", 1)
    for r, k, xs in _chromosomes(name):
        lane = co.lane_partition(xs, beta, m, "kernel")
        for other in (co.partition(xs, beta, m), co.partition_vectorised(xs, beta, m)):
            assert np.asarray(lane[0]).tobytes() == np.asarray(other[0]).tobytes(), (r, k)  # F bit for bit
            assert lane[1] == other[1], (r, k)


@functools.lru_cache(maxsize=None)
def _rows_a_mutant_changes(name, mode):
    """The rows of a named case whose starts or levels (bytes) differ when rule 3 is taken from the lane model in
    ``mode``."""
    c = co.expected(name)
    got = co.cnv_changepoints(c["x"], c["chr_pos"], part=functools.partial(co.lane_partition, mode=mode), **c["kwargs"])
    want = c["want"]
    differs = (got["starts"] != want["starts"]).any(axis=1)
    differs |= (got["levels"].view(np.int64) != want["levels"].view(np.int64)).any(axis=1)
    return np.flatnonzero(differs).tolist()


@pytest.mark.parametrize("name", co.EDGE_CASES + co.TIES_CASES[:3])
def test_the_lane_model_gives_the_oracles_bytes(name):
    assert _rows_a_mutant_changes(name, "kernel") == []


@pytest.mark.parametrize("name, mode", [("ties_long", "lane_le"), ("ties_long", "lowest_lane"), ("ties_long_m2", "lane_le"),
                                        ("ties_long_m2", "lowest_lane"), ("ties_long_m3_beta_eighth", "lowest_lane"),
                                        ("clamp_constant_rows", "no_clamp"), ("clamp_constant_rows_tiny_beta", "no_clamp")]
                         + [(name, "highest_i") for name in co.TIES_CASES if name not in co.TIES_CASES_WITHOUT_A_TIE])
def test_every_mutant_of_the_lane_model_is_told_apart_by_its_case(name, mode):
    """A kernel that made the mistake ``mode`` would fail the GPU comparison of ``name``: the mutant's starts or levels
    differ from the oracle's in at least one row."""
    rows = _rows_a_mutant_changes(name, mode)
    print(f"{name}: {mode} changes the rows {rows}")
    assert len(rows) >= 1


def test_the_short_ties_case_cannot_tell_the_lanes_apart():
    """Why the long cases exist: with at most 16 windows every lane has one candidate, in lanes 0 .. 15, where the lowest
    lane is the lowest i -- neither mutant changes a byte of any of the three short cases."""
    for name in co.TIES_CASES[:3]:
        assert max(np.diff(co.bounds(co.expected(name)["chr_pos"], co.expected(name)["x"].shape[1]))) <= 16
        assert _rows_a_mutant_changes(name, "lane_le") == [] and _rows_a_mutant_changes(name, "lowest_lane") == []


@pytest.mark.parametrize("name", co.TIES_CASES_WITHOUT_A_TIE)
def test_a_beta_that_is_no_multiple_of_a_quarter_leaves_no_tie_to_break(name):
    """beta = c log(W) of "ties", "ties_m3" and "ties_long_m3" (sigma and penalty given, W = 45 or 458): F_j = cost + k beta
    is rounded, two segmentations of one cost are rounded differently, and on these rows the best segmentation is the only
    one in float64 -- not one candidate on the backtracked path equals the chosen one, so no rule for ties, right or wrong,
    changes a byte.  "ties_long_m3_beta_eighth" is the m = 3 case with ties."""
    c = co.expected(name)
    beta, m = c["want"]["beta"], c["kwargs"].get("min_windows", 1)
    assert beta > 0 and beta * 4 != round(beta * 4)
    for mode in ("lane_le", "lowest_lane", "highest_i"):
        assert _rows_a_mutant_changes(name, mode) == []
    for r, k, xs in _chromosomes(name):  # the same, seen directly: the candidates of every j on the path
        F, back, P = co.partition(xs, beta, m)
        Q = co.prefix_chains(xs)[1]
        for i, j in co.backtrack(back, len(xs)):
            equal = [t for t in range(j) if co.admissible(t, j, len(xs), m)
                     and (F[t] + co.segment_cost(P, Q, t, j)) + beta == F[j]]
            assert equal == [i], (r, k, j)


def test_the_limit_cases_hold_what_they_are_named_for():
    lengths = lambda name: np.diff(co.bounds(co.expected(name)["chr_pos"], co.expected(name)["x"].shape[1])).tolist()
    for name in ("ties_long", "ties_long_m2", "ties_long_m3", "ties_long_m3_beta_eighth"):
        assert lengths(name) == [65, 129, 200, 64] and co.expected(name)["x"].shape[0] == 14
    assert co.expected("ties_long")["want"]["beta"] == 0.0 == co.expected("ties_long_m2")["want"]["beta"]
    assert co.expected("ties_long_m3_beta_eighth")["want"]["beta"] == 0.125
    # the existing cases keep their bytes: exact_ties() without lengths is what it was
    x, chr_pos = co.exact_ties()
    assert x.shape == (14, 45) and sorted(chr_pos.values()) == [0, 12, 19, 20, 29]
    assert (co.exact_ties((12, 7, 1, 9, 16))[0] != x).nnz == 0

    # the clamp: twelve rows over 65 and 130 windows, beta = 0 and a beta of 5e-20
    c = co.expected("clamp_constant_rows")
    assert lengths("clamp_constant_rows") == [65, 130] and c["x"].shape == (12, 195) and c["want"]["beta"] == 0.0
    dense = c["x"].toarray()
    assert (dense[:6] == np.asarray(co.CLAMP_VALUES)[:, None]).all()
    assert (dense[6:, :32] == dense[:6, :32]).all() and (dense[6:, 32:65] == 3 * dense[:6, 32:65]).all()
    assert (dense[6:, 65:130] == dense[:6, 65:130]).all() and (dense[6:, 130:] == 3 * dense[:6, 130:]).all()
    tiny = co.expected("clamp_constant_rows_tiny_beta")["want"]["beta"]
    assert tiny == (1.0 * (1e-10 * 1e-10)) * math.log(195) == co.penalty_of(1.0, 1e-10, 195) and 5.2e-20 < tiny < 5.3e-20
    fired = sum(1 for _, _, xs in _chromosomes("clamp_constant_rows") for P, Q in [co.prefix_chains(xs)]
                for j in range(1, len(xs) + 1) for i in range(j)
                if (Q[j] - Q[i]) - ((P[j] - P[i]) * (P[j] - P[i])) / float(j - i) < 0.0)
    assert fired > 1000  # (the costs below 0.0 that the clamp meets)

    # a unique minimum in every lane, in three rounds of k
    c = co.expected("minimum_in_every_lane")
    w = co.EVERY_LANE_WINDOWS
    assert c["x"].shape == (w - 1, w) == (130, 131) and lengths("minimum_in_every_lane") == [w]
    assert c["want"]["beta"] == (1.0 * (0.25 * 0.25)) * math.log(w)
    lanes, rows = set(), co.rows_of(c["x"])
    for r in range(1, w):
        xs = rows[r - 1]
        assert xs == [0.0] * r + [1.0] * (w - r)
        F, back, P = co.partition(xs, c["want"]["beta"], 1)
        Q = co.prefix_chains(xs)[1]
        v = [(F[i] + co.segment_cost(P, Q, i, w)) + c["want"]["beta"] for i in range(w)]
        assert back[w] == r and sorted(v)[0] == v[r] < sorted(v)[1]  # candidate k = i = r, and no other equals it
        assert np.flatnonzero(c["want"]["starts"][r - 1]).tolist() == [0, r]
        lanes.add((r % co.LANES, r // co.LANES))
    assert {lane for lane, _ in lanes} == set(range(co.LANES)) and {t for _, t in lanes} == {0, 1, 2}
    assert all((lane, 1) in lanes for lane in range(co.LANES))  # the second round of k meets every lane

    # values at the bound of rule 7
    c = co.expected("values_at_the_refusal_bound")
    a, w = co.REFUSAL_BOUND_A, co.REFUSAL_BOUND_WINDOWS
    dense = c["x"].toarray()
    assert dense.shape == (5, w) and lengths("values_at_the_refusal_bound") == [w] and c["want"]["beta"] == 0.0
    assert np.abs(dense).max() == a and 4e306 < (a * w) * (a * w) < math.inf and math.isfinite((a * a) * w)
    assert set(np.unique(np.abs(dense[:3]))) == {0.0, a / 2, a}
    assert 0 < 1e-160 * 1e-160 < 2.3e-308 and 5e-324 * 5e-324 == 0.0  # subnormal squares, and squares that vanish
    assert np.isfinite(c["want"]["levels"]).all()
    assert c["want"]["n_segments"][4] == 1 and (c["want"]["n_segments"][:4] > 10).all()
    co.check_values(co.rows_of(c["x"]), 0.0)  # accepted
    dense[0, 0] = 3e152
    with pytest.raises(ValueError, match="magnitude 3e\\+152"):
        co.check_values(co.rows_of(dense), 0.0)
    with pytest.raises(ValueError, match="magnitude 3e\\+152"):
        co.cnv_changepoints(dense, c["chr_pos"], **c["kwargs"])


def test_shuffled_rows_hold_the_same_matrix_in_another_order():
    for name in ("mixed_n3", "ties_long"):
        x = co.expected(name)["x"]
        indptr, indices, data = co.shuffled_rows(x, seed=5)
        assert (indptr == x.indptr).all() and indices.dtype == np.int32 and data.dtype == np.float64
        out_of_order = 0
        for r in range(x.shape[0]):
            a, b = indptr[r], indptr[r + 1]
            assert len(set(indices[a:b].tolist())) == b - a  # unique columns
            order = np.argsort(indices[a:b], kind="stable")
            assert (indices[a:b][order] == x.indices[a:b]).all() and data[a:b][order].tobytes() == x.data[a:b].tobytes()
            out_of_order += int((np.diff(indices[a:b]) < 0).any())
        assert out_of_order >= x.shape[0] - 2  # (an empty row or a row of one entry cannot be out of order)


# ---- the planted case ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_result(seed):
    c = co.planted(seed)
    return c, co.cnv_changepoints(c["x"], c["chr_pos"])


@pytest.mark.parametrize("seed", range(5))
def test_the_planted_levels_and_breakpoints_are_found(seed):
    """6 rows x 270 windows, four planted events of +0.3, +0.6, -0.3 and +0.6 in four chromosomes, noise 0.1, defaults:
    in seeds 0-4 the estimate of sigma lies in [0.113, 0.121], all 72 true segments and no other are found, every
    breakpoint within 2 windows of its planted one, every level within 0.095 of its planted one, and 1 to 5 of the 1 620
    windows are off by more than 0.15."""
    c, got = planted_result(seed)
    f = co.planted_figures(c["truth"], got["levels"], got["starts"])
    print(f"seed {seed}: sigma = {got['sigma']:.4f}, beta = {got['beta']:.4f}, {f}")
    assert 0.11 <= got["sigma"] <= 0.125  # (the noise is 0.1; the few differences across a breakpoint add the rest)
    assert f["n_segments"] == co.PLANTED_SEGMENTS == int(got["n_segments"].sum()) == len(got["table"])
    assert f["shift"] <= 2
    assert f["mean_error"] <= 0.1
    assert f["off"] <= 5
    # what the three-state calls cannot tell apart: the one-copy and the two-copy gain
    assert (got["levels"][:, 115] - got["levels"][:, 35]).min() > 0.2


def test_the_rms_sigma_would_count_the_shifts_as_noise():
    c, got = planted_result(0)
    rms = math.sqrt(float((c["x"] ** 2).mean()))
    assert got["sigma"] < 0.125 < 0.2 < rms


# ---- the library and the package, as far as they go without a GPU -----------------------------------------------------------
def test_symbols_are_exported_and_declared():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_changepoint_levels", "icv_changepoint_diffsq"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+ICV_CHANGEPOINT_MAX_CHR_WINDOWS\s+4096\b", header)
    assert _lib.ICV_CHANGEPOINT_MAX_CHR_WINDOWS == co.MAX_CHR_WINDOWS == 4096
    assert "cnv_changepoints" in cnv.tl.__all__ and callable(cnv.tl.cnv_changepoints)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first
    bad = _lib.ICV_ERR_INVALID
    m = _lib.Matrix()
    m.format, m.dtype, m.n_rows, m.n_cols, m.ld, m.values = _lib.ICV_DENSE, _lib.ICV_F64, 4, 5, 5, 8
    ref = ctypes.byref(m)
    levels, diffsq = lib.icv_changepoint_levels, lib.icv_changepoint_diffsq
    assert levels(None, one, 2, 0.1, 1, one, one, None) == bad
    assert levels(ref, None, 2, 0.1, 1, one, one, None) == bad
    assert levels(ref, one, 2, 0.1, 1, None, one, None) == bad
    assert levels(ref, one, 2, 0.1, 1, one, None, None) == bad
    assert levels(ref, one, 0, 0.1, 1, one, one, None) == bad
    assert levels(ref, one, -1, 0.1, 1, one, one, None) == bad
    assert levels(ref, one, 6, 0.1, 1, one, one, None) == bad  # more chromosomes than windows
    assert levels(ref, one, 2, -0.1, 1, one, one, None) == bad
    assert levels(ref, one, 2, math.nan, 1, one, one, None) == bad
    assert levels(ref, one, 2, math.inf, 1, one, one, None) == bad
    assert levels(ref, one, 2, 0.1, 0, one, one, None) == bad
    assert levels(ref, one, 2, 0.1, -3, one, one, None) == bad
    assert diffsq(None, one, 2, one, None) == bad
    assert diffsq(ref, None, 2, one, None) == bad
    assert diffsq(ref, one, 2, None, None) == bad
    assert diffsq(ref, one, 0, one, None) == bad
    assert diffsq(ref, one, 6, one, None) == bad
    for field, value in (("n_cols", 0), ("n_rows", -1), ("dtype", 7), ("format", 7), ("ld", 4), ("values", None)):
        keep = getattr(m, field)
        setattr(m, field, value)
        assert levels(ref, one, 2, 0.1, 1, one, one, None) == bad, field
        assert b"changepoint_levels" in lib.icv_last_error()
        assert diffsq(ref, one, 2, one, None) == bad, field
        assert b"changepoint_diffsq" in lib.icv_last_error()
        setattr(m, field, keep)
    m.format, m.indptr = _lib.ICV_CSR, None
    assert levels(ref, one, 2, 0.1, 1, one, one, None) == bad  # a CSR matrix without row offsets
    assert diffsq(ref, one, 2, one, None) == bad
    m.n_rows = 0
    assert levels(ref, one, 2, 0.1, 1, one, one, None) == _lib.ICV_OK  # no rows: nothing runs
    assert diffsq(ref, one, 2, one, None) == _lib.ICV_OK


# ---- what the function refuses before it touches the device ---------------------------------------------------------------------
def _adata(n=6, w=10, x=None, chr_pos=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32), obs=pd.DataFrame({"clone": list("aabbcc")[:n]}))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


W = "tl.cnv_changepoints: "
BAD = [
    ("missing obsm key", {"use_rep": "other"}, {}, KeyError, W + "X_other not found in adata.obsm. Did you run `tl.infercnv`?"),
    ("1-D", {}, {"x": np.ones(6)}, ValueError, W + "X must be 2-D"),
    ("no windows", {}, {"x": np.ones((6, 0))}, ValueError, W + "empty matrix of shape (6, 0)"),
    ("chr_pos outside", {}, {"chr_pos": {"chr1": 0, "chr2": 10}}, ValueError, W + "chr_pos start 10 is outside [0, 10)"),
    ("chr_pos empty", {}, {"chr_pos": {}}, ValueError, W + "chr_pos is empty"),
    ("chr_pos without 0", {}, {"chr_pos": {"chr1": 2}}, ValueError, W + "no chromosome of chr_pos starts at window 0"),
    ("chr_pos twice", {}, {"chr_pos": {"chr1": 0, "chr2": 3, "chr3": 3}}, ValueError,
     W + "two chromosomes of chr_pos start at the same window"),
    ("chromosome above the cap", {}, {"n": 2, "x": sp.csr_matrix((2, 4200)), "chr_pos": {"chr1": 0, "chr2": 4097}}, ValueError,
     W + "a chromosome of 4097 windows; the kernel keeps one chromosome in LDS and takes at most 4096 windows"),
    ("penalty=-1", {"penalty": -1}, {}, ValueError, W + "penalty=-1 must be finite and >= 0"),
    ("penalty=nan", {"penalty": math.nan}, {}, ValueError, W + "penalty=nan must be finite and >= 0"),
    ("penalty=inf", {"penalty": math.inf}, {}, ValueError, W + "penalty=inf must be finite and >= 0"),
    ("penalty=True", {"penalty": True}, {}, ValueError, W + "penalty=True must be finite and >= 0"),
    ("penalty='x'", {"penalty": "x"}, {}, ValueError, W + "penalty='x' must be a number"),
    ("sigma=0", {"sigma": 0}, {}, ValueError, W + "sigma=0 must be finite and > 0"),
    ("sigma=-1", {"sigma": -1.0}, {}, ValueError, W + "sigma=-1.0 must be finite and > 0"),
    ("sigma=inf", {"sigma": math.inf}, {}, ValueError, W + "sigma=inf must be finite and > 0"),
    ("sigma='x'", {"sigma": "x"}, {}, ValueError, W + "sigma='x' must be a number"),
    ("min_windows=0", {"min_windows": 0}, {}, ValueError, W + "min_windows=0 must be an integer >= 1"),
    ("min_windows=1.5", {"min_windows": 1.5}, {}, ValueError, W + "min_windows=1.5 must be an integer >= 1"),
    ("min_windows=True", {"min_windows": True}, {}, ValueError, W + "min_windows=True must be an integer >= 1"),
    # the order of the checks: the earlier one speaks
    ("cap before penalty", {"penalty": -1}, {"n": 2, "x": sp.csr_matrix((2, 4200)), "chr_pos": {"chr1": 0}}, ValueError,
     W + "a chromosome of 4200 windows; the kernel keeps one chromosome in LDS and takes at most 4096 windows"),
    ("penalty before sigma", {"penalty": -1, "sigma": 0, "min_windows": 0}, {}, ValueError,
     W + "penalty=-1 must be finite and >= 0"),
    ("sigma before min_windows", {"sigma": 0, "min_windows": 0}, {}, ValueError, W + "sigma=0 must be finite and > 0"),
]


@pytest.mark.parametrize("cid, kw, data, kind, message", BAD, ids=[c[0] for c in BAD])
def test_every_bad_argument_has_its_exception_and_its_whole_message(cid, kw, data, kind, message):
    import infercnvpy_amd as cnv

    ad = _adata(**data)
    with pytest.raises(kind) as info:
        cnv.tl.cnv_changepoints(ad, **kw)
    assert type(info.value) is kind and info.value.args[0] == message
    assert set(ad.obsm) == {"X_cnv"} and list(ad.obs.columns) == ["clone"] and set(ad.uns) == {"cnv"}


def test_a_missing_chr_pos_is_a_key_error():
    import infercnvpy_amd as cnv

    ad = _adata()
    ad.uns["cnv"] = {}
    with pytest.raises(KeyError) as info:
        cnv.tl.cnv_changepoints(ad)
    assert info.value.args[0] == W + "chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"
    del ad.uns["cnv"]
    with pytest.raises(KeyError):
        cnv.tl.cnv_changepoints(ad)
    assert set(ad.obsm) == {"X_cnv"} and set(ad.uns) == set()


def test_chromosome_bounds_keeps_its_messages_for_the_other_callers():
    from infercnvpy_amd.tl._hmm import chromosome_bounds

    with pytest.raises(ValueError) as info:
        chromosome_bounds({}, 5)
    assert info.value.args[0] == "tl.cnv_states: chr_pos is empty"
    assert chromosome_bounds({"b": 3, "a": 0}, 5, "who").tolist() == [0, 3, 5]

"""The exact smoothing cases of ``tests/_smooth_cases.py`` checked on the CPU: the float64 oracle reproduces the table
bit for bit, the restated bin maps put every case where its name says, and the three-FMA quotient of ``finish_window``
is the correctly rounded division on dyadic sums.  (The GPU side is ``tests/test_gpu_smooth_edges.py``.)"""
import os
import re

import numpy as np
import pytest

import _smooth_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("L100", "L100_odd", "L250")


def test_layout_table():
    """The layout of DESIGN.md 4.1: 15 chromosomes + 3 genes without one, the window counts every case needs."""
    L = sc.layout("L100")
    assert L.genes == [735, 745, 425, 415, 405, 1095, 1105, 335, 325, 57, 115, 125, 145, 165, 205]
    assert L.counts == [64, 65, 33, 32, 31, 100, 101, 24, 23, 1, 2, 3, 5, 7, 11]
    assert (L.G, L.W, L.k1, L.k2) == (6400, 502, 250, 251)
    Lo = sc.layout("L100_odd")
    assert Lo.genes[-1] == 100 and Lo.counts[-1] == 1 and (Lo.W, Lo.k1, Lo.k2) == (503, 251, 251)
    L2 = sc.layout("L250")
    assert L2.genes[:15] == [57 if m == 1 else 255 + 10 * (m - 1) for m in L.counts] and sum(L2.genes[:15]) + 3 == 8500
    assert L2.genes[15:] == [250] * 34 and L2.counts[15:] == [1] * 34 and (L2.G, L2.W, L2.k1, L2.k2) == (17000, 536, 267, 268)
    for lay in (L, Lo, L2):
        assert not np.array_equal(lay.chromosome[:-3], np.sort(lay.chromosome[:-3].astype(str)))  # permuted columns


def test_plan_agrees_with_the_layout():
    """The library's host plan (no GPU needed) gives the same window count and first windows."""
    from infercnvpy_amd._plan import GenePlan

    for name in LAYOUTS:
        L = sc.layout(name)
        plan = GenePlan(L.chromosome, L.start, window_size=L.window, step=L.step)
        assert plan.n_windows == L.W
        assert [int(plan.chr_pos[f"chr{c + 1}"]) for c in range(L.n_chr)] == L.first.tolist()
        _, ln = plan.window_table()
        assert {abs(x) for x in ln.tolist()} <= {L.window, sc.FLAT_GENES}, set(ln.tolist())


@pytest.mark.parametrize("name", LAYOUTS)
def test_oracle_equals_the_table_bit_for_bit(name):
    """Windows, median and x_res of every median case: ``infercnv_chunk`` of the float64 oracle against the table."""
    L = sc.layout(name)
    cs = sc.median_cases(name)
    cells = [sc.table_cell(L, c.values) for c in cs]
    X = np.stack([c.x for c in cells])
    win, med, res, _ = sc.oracle_rows(L, X)
    assert np.array_equal(win, np.stack([c.windows for c in cells]))
    assert np.array_equal(med, np.array([c.median for c in cells]))
    assert np.array_equal(res, np.stack([c.x64 for c in cells]))
    assert np.array_equal(res.astype(np.float32), np.stack([c.x_res for c in cells]))
    for c in cells:  # the exact moments are those of the float64 values
        assert c.s == float(np.sum(c.x64.astype(np.longdouble))) and abs(c.q - float((c.x64 ** 2).sum())) <= 1e-12 * c.q


def test_oracle_threshold_equals_the_restated_formula():
    """``dynamic_threshold * np.std`` of the oracle against the library's formula on the exact table moments: the
    population variance written two ways, equal to rounding."""
    L = sc.layout("L100")
    cells = [sc.table_cell(L, c.values) for c in sc.median_cases("L100")[:20]]
    s, q = sc.chunk_moments_exact(cells)
    _, _, _, thr = sc.oracle_rows(L, np.stack([c.x for c in cells]), dynamic_threshold=1.5)
    assert abs(sc.chunk_thr(s, q, len(cells), L.W, 1.5) - thr) <= 1e-12 * thr


@pytest.mark.parametrize("name", LAYOUTS)
def test_cases_are_what_their_names_say(name):
    """Under the x16 map of the layout and under the 4096-bin map: the plateaus lie in the claimed bins, the middle
    ranks sit on the claimed plateau edges, and the median bins hold the claimed number of windows."""
    L = sc.layout(name)
    seen = {}
    for which in (f"x{L.fine}", "h4096"):
        for c in sc.median_cases(name):
            seen[(which, c.name)] = sc.check_case(L, c, which)
    for which in (f"x{L.fine}", "h4096"):
        assert seen[(which, "tie64")] == 64 and seen[(which, "tie65")] == 65
        if L.k1 != L.k2:
            for place in ("same_fine", "two_fine", "two_coarse", "seam_pos", "seam_neg", "tail_pos", "tail_neg"):
                assert seen[(which, f"{place}_33_31")] == 64 and seen[(which, f"{place}_33_32")] == 65
                assert seen[(which, f"{place}_1_64")] == 65 and seen[(which, f"{place}_64_1")] == 65
                assert seen[(which, f"{place}_1_2")] == 3 and seen[(which, f"{place}_100_101")] == 201
            for ma, mb in sc.PAIRS:  # the clipped plateau holds every window on its side of the median
                assert seen[(which, f"last_bin_{ma}_{mb}")] == ma + L.W - L.k2
                assert seen[(which, f"first_bin_{ma}_{mb}")] == mb + L.k1 + 1


def test_bin_maps_at_known_points():
    """The restated maps at points whose bins follow from the kernels' constants by hand."""
    for fine, m in ((1024, sc.MAPS["x1024"]), (4096, sc.MAPS["x4096"]), (4096, sc.MAPS["h4096"])):
        T = fine // 8
        assert m(0.0)[0] == fine // 2 and m(3.0)[0] == fine - 1 and m(-3.0)[0] == 0
        assert m(5.0)[0] == fine - 1 and m(-5.0)[0] == 0  # (beyond the bound: the clamps)
        assert m(0.375)[0] == fine - T - 1 and m(-0.375)[0] == T
        assert m(0.375 + 2.0 ** -10)[0] == fine - T and m(-0.375 - 2.0 ** -10)[0] == T - 1
        v = np.linspace(-3.0, 3.0, 20001)
        assert (np.diff(m(v)) >= 0).all()  # monotone
    # plateau values the cases choose themselves keep 0.1 bin from every edge
    for _, lo, hi in sc.PLACES[5:7]:
        assert sc.is_safe(lo)
    assert sc.is_safe(sc.TIE_VALUE) and sc.is_safe(0.0) and not sc.is_safe(2.0 ** -10)


def test_mixed_matrix_covers_every_neighbourhood():
    """The pipeline matrix at a small CU count: every ordered pair of cell types at grids cu, 2 cu, 4 cu, every triple
    at grid cu (asserted by the builder), a third of each type."""
    cu = 16
    mx = sc.mixed_matrix("L100", cu, 10)
    assert len(mx.kind) == 159 and [(mx.kind == k).sum() for k in (0, 1, 2)] == [53, 53, 53]
    assert np.isnan(mx.X).sum() == 53 and np.isnan(mx.X[mx.kind == sc.NAN]).sum(axis=1).tolist() == [1] * 53
    L = sc.layout("L100")
    for r in np.flatnonzero(mx.kind == sc.HANDED):
        assert sc.handed_back(L, mx.windows[r], "x16") and sc.handed_back(L, mx.windows[r], "se")
        assert mx.stats[r, 1] > 0
    assert not sc._adjacency_ok(np.repeat(np.array([0, 1, 2]), 53), cu)  # (the check can fail: sorted types do)


@pytest.mark.parametrize("den", [2500, 2550, 15625, 15750])
def test_three_fma_quotient_is_the_ieee_division_on_dyadic_sums(den):
    """``finish_window``: q = acc * rcp, one residual step.  On sums of multiples of 2^-4 with |value| <= 3 (what a
    window of a dyadic cell accumulates; 2550 and 15750 are the pyramid sums of windows 100 and 250) the result is
    the correctly rounded ``acc / den`` -- numpy's division, which the oracle uses."""
    rng = np.random.default_rng(den)
    acc = rng.integers(-3 * den * 16, 3 * den * 16 + 1, 6000) / 16.0
    acc = np.concatenate([acc, [0.0, 3.0 * den, -3.0 * den, 1 / 16.0, den / 16.0, (den - 1) / 16.0]])
    want = acc / float(den)
    got = np.array([sc.fma3_quotient(float(a), den) for a in acc])
    assert np.array_equal(got, want)
    # the weighted sum of a constant window is exact and its quotient is the constant again
    v = rng.integers(-3 * 2 ** 14, 3 * 2 ** 14 + 1, 2000) / 2.0 ** 14
    assert np.array_equal(np.array([sc.fma3_quotient(float(x * den), den) for x in v]), v)
    assert np.array_equal((v * den) / den, v)


def test_accessor_is_declared_exported_and_checks_its_arguments():
    """``icv_plan_last_handed_back``: in the header, in ``_lib.EXPORTS``, in the library; NULL arguments are refused and
    a plan that has launched nothing reports 0 (no GPU needed for either)."""
    import ctypes as C

    from infercnvpy_amd import _lib
    from infercnvpy_amd._plan import GenePlan

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    name = "icv_plan_last_handed_back"
    assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert "int icv_plan_last_handed_back(icv_plan_t plan, int64_t *h_n);" in header
    L = sc.layout("L100")
    plan = GenePlan(L.chromosome, L.start, window_size=L.window, step=L.step)
    n = C.c_int64(-1)
    assert lib.icv_plan_last_handed_back(None, C.byref(n)) == _lib.ICV_ERR_INVALID
    assert lib.icv_plan_last_handed_back(plan.handle, None) == _lib.ICV_ERR_INVALID
    assert plan.last_kernel() == _lib.ICV_KERNEL_NONE and plan.last_handed_back() == 0

"""``k_smooth_x16``, ``k_smooth_ws``, ``k_smooth_se`` and the generic ``k_smooth`` pinned at their median, hand-back,
pipeline and chunk limits, on the exact inputs of ``tests/_smooth_cases.py`` (``-m gpu``).

Routes through ``_engine.run_hot_path`` (the kernel that ran is asserted through ``plan.last_kernel()``, the number of
cells it handed back through ``plan.last_handed_back()``):

    x16      dense float32, default
    ws       dense float32, developer knob ICV_NO_X16
    generic  dense float32, developer knob ICV_FORCE_GENERIC
    se       float32 CSR of the same matrix, default

x16, ws and generic keep the canonical float64 order: ``out``, ``cell_median``, the float64 windows and -- on
piecewise-constant cells, whose sums are exact in any order -- ``cell_stats`` and the thresholds equal the table bit for
bit.  se sums in fixed point in another order: on the dyadic cells of the pipeline matrix it is held to the bounds the
project states for it (``out`` 2.5e-7, ``cell_median`` 1e-11; moments 1e-9); on piecewise-constant cells it is exact
as well (measured, then asserted: TABLE_EXACT), and the cells it hands back are recomputed by ``k_smooth``.

Two settings of the library shape the calls: the float64 windows are written by x16 and se only in chunk-moment mode
(``cell_stats=None``) -- with ``cell_stats=True`` and ``windows=True`` every route runs the generic kernel -- and ws never
writes them.  So every route is run with ``cell_stats=True`` (per-cell moments) and, where it has one, again with
``cell_stats=None, windows=True`` (chunk moments + windows).
"""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _smooth_cases as sc

pytestmark = pytest.mark.gpu

ROUTES = ("x16", "ws", "generic", "se")
ENV = {"x16": (), "ws": ("ICV_NO_X16",), "generic": ("ICV_FORCE_GENERIC",), "se": ()}
EXACT = {"x16": True, "ws": True, "generic": True, "se": False}
SE_OUT, SE_MED, SE_MOM = 2.5e-7, 1e-11, 1e-9  # the project's bounds for the stored-entries kernel's other order
# On piecewise-constant cells the fixed-point sums of k_smooth_se are exact too (every entry's difference to the zero
# row is a multiple of 2^-14, every prefix sum fits its bin): measured equal to the table in every bit of out,
# cell_median, cell_stats and the windows, so equality is what the table tests assert on ALL routes.  The tolerances
# above remain for the dyadic cells of the pipeline tests, whose window quotients se forms from other partial sums.
TABLE_EXACT = True
_PLANS = {}


def _cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _plan(L):
    from infercnvpy_amd._plan import GenePlan

    if L.name not in _PLANS:
        _PLANS[L.name] = GenePlan(L.chromosome, L.start, window_size=L.window, step=L.step)
    return _PLANS[L.name]


def _kernel_of(route):
    from infercnvpy_amd import _lib

    return {"x16": _lib.ICV_KERNEL_X16, "ws": _lib.ICV_KERNEL_WS, "generic": _lib.ICV_KERNEL_GENERIC,
            "se": _lib.ICV_KERNEL_SD}[route]


class Route:
    """One route on one matrix: sets the developer knobs for the calls made inside ``with``."""

    def __init__(self, monkeypatch, L, X, route, plan=None):
        import torch

        from infercnvpy_amd import _engine

        self.mp, self.L, self.route, self.plan = monkeypatch, L, route, plan or _plan(L)
        self.ref = torch.from_numpy(L.ref).cuda()
        self.dm = _engine.to_device_matrix(sp.csr_matrix(X) if route == "se" else X)
        self.n = X.shape[0]

    def __enter__(self):
        from infercnvpy_amd import _lib

        for k in ("ICV_FORCE_GENERIC", "ICV_NO_X16", "ICV_NO_SD"):
            self.mp.delenv(k, raising=False)
        for k in ENV[self.route]:
            self.mp.setenv(k, "1")
        _lib.load().icv_developer_knobs_reload()
        return self

    def __exit__(self, *exc):
        from infercnvpy_amd import _lib

        for k in ENV[self.route]:
            self.mp.delenv(k, raising=False)
        _lib.load().icv_developer_knobs_reload()
        return False

    def run(self, *, stats, windows=False, dyn=None, chunksize=5000, row_phase=0, row0=0, row1=None):
        """-> dict of host arrays + the number of cells handed back; asserts the kernel of the route ran."""
        import torch

        from infercnvpy_amd import _engine

        res = _engine.run_hot_path(self.plan, self.dm, self.ref, lfc_clip=sc.CLIP, dynamic_threshold=dyn,
                                   chunksize=chunksize, row_phase=row_phase, cell_stats=stats, windows=windows,
                                   row0=row0, row1=row1)
        torch.cuda.synchronize()
        assert self.plan.last_kernel() == _kernel_of(self.route), (self.route, self.plan.last_kernel())
        return dict(out=res.out.cpu().numpy(), median=res.cell_median.cpu().numpy(),
                    stats=None if res.cell_stats is None else res.cell_stats.cpu().numpy(),
                    thr=None if res.thr is None else res.thr.cpu().numpy(),
                    windows=None if res.windows is None else res.windows.cpu().numpy(),
                    handed=self.plan.last_handed_back())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same(got, want, what, exact, tol=None, rel=False):
    """Bit for bit (NaN patterns included) on the canonical routes; within ``tol`` for se."""
    got, want = np.asarray(got), np.asarray(want).astype(got.dtype)
    assert got.shape == want.shape, what
    if got.size == 0:
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN pattern"
    g, w = np.where(gn, 0, got), np.where(wn, 0, want)
    if exact:
        bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{what}: rows {bad[:8]} differ, max |d| {np.abs(g.astype(np.float64) - w).max()}"
    else:
        d = np.abs(g.astype(np.float64) - w.astype(np.float64))
        lim = tol * (1.0 + np.abs(w.astype(np.float64))) if rel else tol  # (rel: rtol = atol = tol)
        assert (d <= lim).all(), f"{what}: max |d| {d.max()} at row {np.unravel_index(d.argmax(), d.shape)[0]}"


def _check(r, route, out, median, stats=None, windows=None, handed_rows=(), what="", exact=None):
    """A result against expected values; the rows the route hands back are exact on every route (``k_smooth``).
    ``exact=True``: piecewise-constant cells, on which k_smooth_se is exact as well (TABLE_EXACT)."""
    ex = EXACT[route] if exact is None else exact
    _same(r["out"], out, f"{what} {route} out", ex, SE_OUT)
    _same(r["median"], median, f"{what} {route} median", ex, SE_MED)
    if stats is not None and r["stats"] is not None:
        _same(r["stats"], stats, f"{what} {route} stats", ex, SE_MOM, rel=True)
    if windows is not None and r["windows"] is not None:
        _same(r["windows"], windows, f"{what} {route} windows", ex, SE_MED)
    hb = np.asarray(handed_rows, dtype=np.int64)
    if not ex and hb.size:
        _same(r["out"][hb], np.asarray(out)[hb], f"{what} {route} handed-back out", True)
        _same(r["median"][hb], np.asarray(median)[hb], f"{what} {route} handed-back median", True)
        if windows is not None and r["windows"] is not None:
            _same(r["windows"][hb], np.asarray(windows)[hb], f"{what} {route} handed-back windows", True)


def _table(L, cells):
    return dict(out=np.stack([c.x_res for c in cells]), median=np.array([c.median for c in cells]),
                stats=np.array([[c.s, c.q] for c in cells]), windows=np.stack([c.windows for c in cells]))


def _has_windows(route):
    return route != "ws"  # k_smooth_ws does not write the float64 windows (the library runs k_smooth for them)


# --------------------------------------------------------------------------------------------------------------- #
# where the median lies, and the 64 / 65 boundary
# --------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["L100", "L100_odd", "L250"])
def test_median_cases(name, route, monkeypatch):
    """Every median case of the layout (``_smooth_cases.median_cases``: one chromosome tying with 64 / 65 windows; two
    plateaus sharing the middle ranks with 33+31, 33+32, 1+64, 64+1, 1+2, 100+101 windows, placed in one fine bin, two
    fine bins, two coarse bins, across either seam, in a tail, in the last and in the first bin) as one matrix and
    row by row: values from the table, and the EXACT number of cells handed back -- nin <= 64 keeps a cell, 65 hands
    it back; in the first / last bin every window beyond the median is clipped to one value, so those cells are
    always handed back."""
    L = sc.layout(name)
    cs = sc.median_cases(name)
    cells = [sc.table_cell(L, c.values) for c in cs]
    t = _table(L, cells)
    X = np.stack([c.x for c in cells])
    handed = np.array([sc.handed_back(L, c.windows, route) for c in cells])
    if route != "generic":  # (both counts occur, or the 64 / 65 boundary is not exercised)
        assert handed.any() and not handed.all()
    hb = np.flatnonzero(handed)
    with Route(monkeypatch, L, X, route) as R:
        r = R.run(stats=True)
        assert r["handed"] == handed.sum(), (r["handed"], [c.name for c, h in zip(cs, handed) if h])
        _check(r, route, t["out"], t["median"], t["stats"], handed_rows=hb, what=name, exact=TABLE_EXACT)
        if _has_windows(route):
            r = R.run(stats=None, windows=True)
            assert r["handed"] == handed.sum()
            _check(r, route, t["out"], t["median"], windows=t["windows"], handed_rows=hb, what=name + " chunk mode",
                   exact=TABLE_EXACT)
        for i, c in enumerate(cs):  # one cell per launch: the count is observed per case
            r = R.run(stats=True, row0=i, row1=i + 1)
            assert r["handed"] == int(handed[i]), (c.name, r["handed"])
            _check(r, route, t["out"][i:i + 1], t["median"][i:i + 1], t["stats"][i:i + 1],
                   handed_rows=[0] if handed[i] else [], what=f"{name} {c.name}", exact=TABLE_EXACT)


# --------------------------------------------------------------------------------------------------------------- #
# hand-back accounting in chunk mode
# --------------------------------------------------------------------------------------------------------------- #
def _accounting_cells(L, names):
    by_name = {c.name: c for c in sc.median_cases(L.name)}
    return [sc.table_cell(L, by_name[n].values) for n in names]


def _expected_thresholded(cells, rows_of_chunk, W, dyn):
    """(thr per chunk, thresholded x_res) from the table; no entry may lie within 1e-6 relative of its threshold."""
    thr, out = [], np.stack([c.x_res for c in cells]).copy()
    for rows in rows_of_chunk:
        s, q = sc.chunk_moments_exact([cells[r] for r in rows])
        th = sc.chunk_thr(s, q, len(rows), W, dyn)
        thr.append(th)
        for r in rows:
            a = np.abs(cells[r].x64)
            assert th > 0 and (np.abs(a - th) > 1e-6 * th).all(), "an entry sits on the threshold"
            out[r][a < th] = 0.0
    return np.array(thr), out


@pytest.mark.parametrize("route", ROUTES)
def test_hand_back_accounting(route, monkeypatch):
    """``cell_stats=None`` with thresholds: a cell handed back is skipped by the fast kernel's chunk moments and comes
    back through the plan's per-row buffer.  The handed-back cells carry more than 10 % of a chunk's sum of squares,
    so dropping or doubling one moves the threshold by percent; asserted: thr against the formula on the exact table
    moments (rtol 1e-12), thr of the per-cell mode bit for bit (the sums are exact in any order), the zero pattern of
    the thresholded output, and that a second, shorter call on the same plan -- which hands back no cell, or other
    cells -- gives its own values and not those left behind by the first."""
    L = sc.layout("L100")
    dyn, cs = 1.5, 7
    first = ["tie65", "same_fine_1_2", "two_coarse_33_32", "tie64", "seam_pos_1_64", "two_fine_33_31", "tail_pos_64_1",
             "same_fine_33_31", "two_fine_1_2", "last_bin_1_2", "seam_neg_33_31", "two_coarse_1_2", "tail_neg_100_101",
             "seam_pos_1_2", "tie64", "first_bin_33_31", "tail_pos_33_31", "same_fine_100_101", "two_coarse_33_31"]
    second_none = ["tie64", "two_fine_1_2", "seam_neg_33_31", "same_fine_33_31", "tail_pos_33_31", "two_coarse_1_2",
                   "seam_pos_1_2", "two_fine_33_31", "tie64", "same_fine_1_2", "two_coarse_33_31"]
    second_other = ["tie64", "two_fine_1_2", "tie65", "same_fine_33_31", "tail_pos_33_31", "two_coarse_100_101",
                    "seam_pos_1_2", "two_fine_33_31", "first_bin_1_2"]
    plan = None
    for k, names in enumerate((first, second_none, first, second_other)):
        cells = _accounting_cells(L, names)
        X = np.stack([c.x for c in cells])
        handed = np.array([sc.handed_back(L, c.windows, route) for c in cells])
        chunks = sc.chunk_rows(len(cells), cs, 0)
        if route != "generic":
            assert handed.sum() == {0: 8, 1: 0, 2: 8, 3: 3}[k]
            for rows in chunks:  # the share of the handed-back cells in the chunk's sum of squares
                q_hb = sum(cells[r].q for r in rows if handed[r])
                assert not handed[rows].any() or q_hb >= 0.1 * sum(cells[r].q for r in rows)
        thr, out = _expected_thresholded(cells, chunks, L.W, dyn)
        with Route(monkeypatch, L, X, route, plan) as R:
            plan = R.plan
            lean = R.run(stats=None, dyn=dyn, chunksize=cs)
            full = R.run(stats=True, dyn=dyn, chunksize=cs)
        for r in (lean, full):
            assert r["handed"] == handed.sum()
        np.testing.assert_allclose(lean["thr"], thr, rtol=1e-12, atol=0, err_msg=f"call {k}")
        assert np.array_equal(_bits(lean["thr"]), _bits(full["thr"])), (k, lean["thr"], full["thr"])
        assert np.array_equal(_bits(lean["thr"]), _bits(thr)), "exact moments: the formula gives the same bits"
        for r in (lean, full):
            assert np.array_equal(r["out"] == 0, out == 0), f"call {k}: zero pattern"
            _same(r["out"], out, f"call {k} {route} thresholded out", TABLE_EXACT)
            _same(r["median"], np.array([c.median for c in cells]), f"call {k} {route} median", TABLE_EXACT)


# --------------------------------------------------------------------------------------------------------------- #
# pipeline positions
# --------------------------------------------------------------------------------------------------------------- #
def _check_mixed(r, route, mx, rows, what):
    kind = mx.kind[rows]
    nan = kind == sc.NAN
    assert np.isnan(r["out"][nan]).all() and np.isnan(r["median"][nan]).all(), what
    assert not np.isnan(r["out"][~nan]).any() and not np.isnan(r["median"][~nan]).any(), what
    # k_smooth_se hands a cell with a stored NaN back as well
    want_handed = int((kind == sc.HANDED).sum()) + (int(nan.sum()) if route == "se" else 0)
    assert r["handed"] == (0 if route == "generic" else want_handed), (what, r["handed"], want_handed)
    hb = np.flatnonzero(kind == sc.HANDED)
    _check(r, route, mx.x_res[rows], mx.median[rows], windows=mx.windows[rows], handed_rows=hb, what=what)
    if r["stats"] is not None:
        # piecewise-constant cells: exact sums; dyadic cells: kernel-specific fixed orders, the project's 1e-12
        _same(r["stats"][hb], mx.stats[rows][hb], f"{what} {route} stats of handed-back cells", True)
        plain = np.flatnonzero(kind == sc.PLAIN)
        np.testing.assert_allclose(r["stats"][plain], mx.stats[rows][plain], rtol=1e-12 if EXACT[route] else SE_MOM,
                                   atol=1e-12 if EXACT[route] else SE_MOM, err_msg=what)
        assert np.isnan(r["stats"][nan]).all(), what


PIPELINE = [("L100", r) for r in ROUTES] + [("L250", "x16")]


@pytest.mark.parametrize("name,route", PIPELINE)
def test_pipeline_positions(name, route, monkeypatch):
    """A workgroup has three cells in flight and reuses its parity slots every second cell.  Row counts 1, 2, 3,
    cu - 1, cu, cu + 1, 2 cu + 1, and a matrix of about 10 cu rows (3 cu at window 250) in which plain
    dyadic cells, handed-back cells and NaN cells follow each other in every order inside a workgroup's sequence
    (asserted by the builder for grids of cu, 2 cu and 4 cu workgroups) and stand first and last in one.  NaN rows are
    all NaN with a NaN median, no other row has a NaN, everything else -- handed-back rows and the float64 windows
    included -- equals the oracle / the table."""
    cu = _cu()
    L = sc.layout(name)
    # (window 250 runs the x16 route only: one workgroup per CU, and 3 cu rows of 17 000 genes are the same 52 MB)
    mx = sc.mixed_matrix(name, cu, 10) if name == "L100" else sc.mixed_matrix(name, cu, 3, grids=(1,))
    n_all = len(mx.kind)
    sizes = [1, 2, 3, cu - 1, cu, cu + 1, 2 * cu + 1, n_all]
    with Route(monkeypatch, L, mx.X, route) as R:
        for n in sizes:
            rows = np.arange(n)
            r = R.run(stats=True, row1=n)
            _check_mixed(r, route, mx, rows, f"{name} n={n} per-cell moments")
            if _has_windows(route):
                r = R.run(stats=None, windows=True, row1=n)
                _check_mixed(r, route, mx, rows, f"{name} n={n} chunk moments + windows")
        # the last rows of the matrix as a launch of their own: other cells come first in their workgroups
        n = 2 * cu + 1
        rows = np.arange(n_all - n, n_all)
        r = R.run(stats=True, row0=n_all - n, row1=n_all)
        _check_mixed(r, route, mx, rows, f"{name} last {n} rows")


# --------------------------------------------------------------------------------------------------------------- #
# chunk boundaries
# --------------------------------------------------------------------------------------------------------------- #
def _cycle_cells(L, n):
    cs = sc.median_cases(L.name)
    cells = [sc.table_cell(L, c.values) for c in cs]
    order = np.random.default_rng(3).permutation(len(cells))
    return [cells[order[i % len(cells)]] for i in range(n)]


@pytest.mark.parametrize("route", ROUTES)
def test_chunk_boundaries(route, monkeypatch):
    """``cell_stats=None`` on ``2 cu + 37`` piecewise-constant cells: chunk sizes 2, 7, cu - 1, cu, cu + 1, n, n + 1
    with row phases 0, 3 and chunksize - 1 -- chunks that start in the middle of a workgroup's sequence, chunks in
    which a workgroup has no cell, one chunk for everything.  Every chunk's threshold equals the formula over exactly
    the rows r with (r + row_phase) // chunksize == k (rtol 1e-12; in fact the same bits: the sums are exact)."""
    cu = _cu()
    L = sc.layout("L100")
    n, dyn = 2 * cu + 37, 1.5
    cells = _cycle_cells(L, n)
    X = np.stack([c.x for c in cells])
    with Route(monkeypatch, L, X, route) as R:
        for cs in (2, 7, cu - 1, cu, cu + 1, n, n + 1):
            for phase in sorted({0, 3, cs - 1}):
                if phase >= cs:
                    continue
                chunks = sc.chunk_rows(n, cs, phase)
                want = np.array([sc.chunk_thr(*sc.chunk_moments_exact([cells[r] for r in rows]), len(rows), L.W, dyn)
                                 for rows in chunks])
                r = R.run(stats=None, dyn=dyn, chunksize=cs, row_phase=phase)
                assert r["thr"].shape == want.shape, (cs, phase)
                np.testing.assert_allclose(r["thr"], want, rtol=1e-12, atol=0, err_msg=f"chunksize {cs} row_phase {phase}")
                assert np.array_equal(_bits(r["thr"]), _bits(want)), (cs, phase)


@pytest.mark.parametrize("route", ["x16", "se"])
def test_chunk_mode_limit(route, monkeypatch):
    """Chunk mode needs ``n_chunks * n_part`` partial-moment slots (n_part = 16 per CU for both kernels) and is used up
    to (64 << 20) / 16 of them; beyond, the library silently forms per-cell moments.  At ``chunksize=1`` that is
    n = 1024 (chunk mode) against n = 1025 (per-cell) on 256 CUs.  Both must give the table's thresholds."""
    cu = _cu()
    L = sc.layout("L100")
    lim = ((64 << 20) // 16) // (16 * cu)
    cells = _cycle_cells(L, lim + 1)
    X = np.stack([c.x for c in cells])
    want = np.array([sc.chunk_thr(c.s, c.q, 1, L.W, 1.5) for c in cells])
    with Route(monkeypatch, L, X, route) as R:
        for n in (lim, lim + 1):
            r = R.run(stats=None, dyn=1.5, chunksize=1, row1=n)
            np.testing.assert_allclose(r["thr"], want[:n], rtol=1e-12, atol=0, err_msg=str(n))
            assert np.array_equal(_bits(r["thr"]), _bits(want[:n])), n


# --------------------------------------------------------------------------------------------------------------- #
# public API
# --------------------------------------------------------------------------------------------------------------- #
def test_public_api_on_the_mixed_matrix():
    """``tl.infercnv`` on the mixed matrix without its NaN cells, from host dense and from host CSR, chunksize 97: the
    zero pattern is the oracle's; the dense route's values are float64(float32(expected)), the CSR route's within
    2.5e-7."""
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData
    from oracle import infercnv_oracle as O

    L = sc.layout("L100")
    mx = sc.mixed_matrix("L100", _cu(), 10)
    rows = np.flatnonzero(mx.kind != sc.NAN)[:1000]
    X = mx.X[rows]
    var = pd.DataFrame({"chromosome": L.chromosome, "start": L.start, "end": L.start + 1000},
                       index=[f"g{i}" for i in range(L.G)])
    _, o_res, _, _ = O.infercnv(X, L.chromosome, L.start, reference=L.ref, chunksize=97)
    want = o_res.toarray()
    keep = want != 0
    assert 0.05 < keep.mean() < 0.95
    exact = np.where(keep, mx.x_res[rows].astype(np.float64), 0.0)  # float64(float32(x64)) where the oracle keeps it
    assert np.abs(exact - want).max() <= 2.5e-7
    for Xin, tol in ((X, 0.0), (sp.csr_matrix(X), SE_OUT)):
        _, res, _ = cnv.tl.infercnv(SimpleAnnData(Xin, var=var), reference=L.ref, chunksize=97, inplace=False)
        got = res.toarray()
        assert got.dtype == np.float64 and np.array_equal(got != 0, keep)
        if tol == 0.0:
            assert np.array_equal(got, exact)
        else:
            assert np.abs(got - exact).max() <= tol

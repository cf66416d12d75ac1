"""The gene-value kernels pinned at their median, run-sum and layout limits (``-m gpu``).

Every case goes through ``_engine.gene_values_from_windows`` on planted float64 windows (``tests/_gene_cases.py``; that
each reaches the branch it is named for is proven on the CPU in ``tests/test_gene_oracle.py``), once on the route the
launcher picks -- ``k_gene_fused`` where the plan admits it -- and once with the developer knob ``ICV_NO_GENE_FUSED``
(``k_gene_means`` -> ``k_row_median`` -> ``k_gene_finish``).  Both must equal the numpy contract of the run tables
(``_gene_oracle.gene_layer``) under ``same_bytes``: identical NaN masks, identical bits after ``+ 0.0``.  No tolerance.
"""
import numpy as np
import pytest

import _gene_cases as gc
import _gene_oracle as go

pytestmark = pytest.mark.gpu

# The launcher's route is restated by hand (there is no entry point that reports it): these numbers and _lds_bytes MUST
# follow csrc/icv_kernel_gene.hpp (struct GvScratch, gv_lds_bytes) and csrc/icv_plan.hpp (kLdsLimit).  If the struct or
# the formula changes and they do not, the `fused` / `pk_lds` assertions below go stale without failing.
GV_SCRATCH_BYTES = 9160  # sizeof(GvScratch): hist 8192 + red 128 + cand_v 512 + cand_w 256 + wsum 32 + 4 ints + v1, v2 + 2 ints
LDS_LIMIT = 160 * 1024   # kLdsLimit
ROUTES = ("default", "round1")
_PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    """The plans are shared by the tests of this file and closed (device tables freed) when it is done."""
    yield
    for plan, _ in _PLANS.values():
        plan.close()
    _PLANS.clear()


def _plan(name):
    if name not in _PLANS:
        plan = gc.make_plan(name)
        _PLANS[name] = (plan, plan.gene_runs())
    return _PLANS[name]


def _lds_bytes(W, R, mult_bytes, pk_lds):
    """gv_lds_bytes of csrc/icv_kernel_gene.hpp."""
    w = max(W * 8, GV_SCRATCH_BYTES)
    w = (w + 15) // 16 * 16
    return w + (R + 2) * 8 + (R * mult_bytes + 15) // 16 * 16 + (R * 4 if pk_lds else 0)


def _launch_shape(plan, runs):
    """-> (fused, mult_bytes, pk_lds) as the launcher decides them (icv_api.hip: gene_from_windows)."""
    W, R = plan.n_windows, len(runs["first"])
    mult_bytes = 2 if runs["genes"].max() > 255 else 1
    pk_lds = _lds_bytes(W, R, mult_bytes, True) * 2 <= LDS_LIMIT
    fused = _lds_bytes(W, R, mult_bytes, pk_lds) <= LDS_LIMIT and runs["count"].max() <= 128
    return fused, mult_bytes, pk_lds


def _device(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _both_routes(monkeypatch, call):
    """call() on the launcher's own route and under ICV_NO_GENE_FUSED -> {route: host array}."""
    import torch

    from infercnvpy_amd import _lib

    got = {}
    for route in ROUTES:
        if route == "round1":
            monkeypatch.setenv("ICV_NO_GENE_FUSED", "1")
            _lib.load().icv_developer_knobs_reload()
        try:
            out = call()
            torch.cuda.synchronize()
            got[route] = out.cpu().numpy()
        finally:
            if route == "round1":
                monkeypatch.delenv("ICV_NO_GENE_FUSED")
                _lib.load().icv_developer_knobs_reload()
    return got


def _check(monkeypatch, name, win, *, thr=None, chunksize=1, row_phase=0, names=None, even_stride=False):
    """The layer of ``win`` (host rows x W) on both routes against the contract.  ``even_stride``: the windows as a view
    into a buffer of even row stride (16-byte loads for an odd W as well)."""
    import torch

    from infercnvpy_amd import _engine

    plan, runs = _plan(name)
    assert win.shape[1] == plan.n_windows
    want = go.gene_layer(runs, win, plan.n_cols_all, thr=thr, chunksize=chunksize, row_phase=row_phase)
    assert np.isnan(want).any(axis=0).sum() >= 10 and not np.isnan(want).all()  # chrX / unplaced columns have no value
    d_win = _device(win)
    if even_stride:
        buf = torch.full((win.shape[0], win.shape[1] + 2 + win.shape[1] % 2), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :win.shape[1]] = d_win
        d_win = buf[:, :win.shape[1]]
        assert d_win.stride(0) % 2 == 0 and d_win.data_ptr() % 16 == 0
    d_thr = None if thr is None else _device(np.asarray(thr, dtype=np.float64))
    got = _both_routes(monkeypatch, lambda: _engine.gene_values_from_windows(
        plan, d_win, thr=d_thr, chunksize=chunksize, row_phase=row_phase, n_vars=plan.n_cols_all))
    for route in ROUTES:
        try:
            go.same_bytes(got[route], want)
        except AssertionError as e:
            row = str(e)
            raise AssertionError(f"plan {name}, route {route}" + (f", rows {names}" if names else "") + ": " + row) from None
    return want


def _planted_matrix(n, with_nan=True):
    pats = gc.planted(n)
    names, mat = gc.shuffled(pats)
    extra = gc.dyadic(4, n, seed=n)
    if with_nan:
        extra[1, n // 3] = np.nan  # a row with one NaN window: NaN in every covered column
        names = names + ["dyadic", "dyadic_nan", "dyadic", "dyadic"]
    else:
        names = names + ["dyadic"] * 4
    return names, np.vstack([mat, extra])


@pytest.mark.parametrize("name", ["odd", "even"])
def test_planted_medians(name, monkeypatch):
    """Crowded bins, refinements, ties, the k2 search, bin 0 / bin 2047, adjacent doubles, 64 / 65 candidates, a NaN
    window: one run per gene, so the row IS the multiset."""
    plan, runs = _plan(name)
    n = len(runs["first"])
    assert (runs["count"] == 1).all() and (runs["genes"] == 1).all() and n == plan.n_windows
    assert _launch_shape(plan, runs) == (True, 1, True)
    names, mat = _planted_matrix(n)
    want = _check(monkeypatch, name, mat, names=names)
    assert np.isnan(want[names.index("dyadic_nan")]).all() and not np.isnan(want[0]).all()
    _check(monkeypatch, name, mat, thr=np.array([0.5, 2.0 ** -12, 0.0, 3.0]), chunksize=len(names) // 4 + 1, names=names)


@pytest.mark.parametrize("name", ["odd", "even"])
def test_zero_and_the_smallest_subnormal(name, monkeypatch):
    """hi - lo = 5e-324: 2048 / (hi - lo) overflows, the bins degenerate to {== lo, > lo}."""
    plan, runs = _plan(name)
    names, mat = gc.shuffled(gc.subnormal(len(runs["first"])))
    _check(monkeypatch, name, mat, names=names)


def test_runs_of_different_lengths(monkeypatch):
    """The weighted median proper: runs of 1..8 genes, rows whose weighted median is not the median of the run values."""
    plan, runs = _plan("weighted")
    assert len(set(runs["genes"])) > 1 and (runs["count"] == 1).all()
    win = gc.dyadic(12, plan.n_windows, seed=3)
    weighted = np.array([np.median(np.repeat(row[runs["first"]], runs["genes"])) for row in win])
    assert (weighted != np.median(win[:, runs["first"]], axis=1)).sum() >= 6
    _check(monkeypatch, "weighted", win)
    win[5, 17] = np.nan
    _check(monkeypatch, "weighted", win, thr=np.array([0.75, 1.5]), chunksize=7, row_phase=2)


@pytest.mark.parametrize("name", ["heavy", "heavy3", "light4"])
def test_a_handful_of_heavy_runs(name, monkeypatch):
    """Runs of 300 genes (16-bit run lengths in LDS) next to a plan whose runs fit a byte; 3, 4 and 6 windows: the scratch
    is larger than the windows.  Rows: every assignment of three values to the windows."""
    plan, runs = _plan(name)
    fused, mult_bytes, pk_lds = _launch_shape(plan, runs)
    assert fused and pk_lds and mult_bytes == (1 if name == "light4" else 2)
    assert plan.n_windows * 8 < GV_SCRATCH_BYTES and plan.n_windows == {"heavy": 6, "heavy3": 3, "light4": 4}[name]
    _check(monkeypatch, name, gc.small_rows(plan.n_windows))


def test_five_thousand_runs(monkeypatch):
    """R = W = 5001: the run table stays in memory (pk_lds off); with 16-byte window loads (an even row stride) the
    windows beyond the two prefetched vectors per thread are loaded in the cell's own loop and the odd last window by
    thread 0; with the odd stride of the contiguous matrix every window is an 8-byte load."""
    plan, runs = _plan("wide")
    n = len(runs["first"])
    assert n == plan.n_windows > 2 * 2 * 512 * 2 and n % 2 == 1 and (runs["count"] == 1).all() and (runs["genes"] == 2).all()
    assert _launch_shape(plan, runs) == (True, 1, False)
    names, mat = _planted_matrix(n)
    _check(monkeypatch, "wide", mat, names=names, even_stride=True)
    _check(monkeypatch, "wide", mat, names=names)


@pytest.mark.parametrize("name", ["rm_even", "rm_odd"])
def test_row_median_limits(name, monkeypatch):
    """k_row_median with more than 1024 covered genes: > 1024 equal values, > 1024 values on one of two adjacent doubles,
    a first pivot between the two middle elements, consecutive doubles that 60 halvings do not separate."""
    plan, runs = _plan(name)
    n = len(runs["first"])
    assert n > 1024 and (runs["count"] == 1).all() and (runs["genes"] == 1).all()
    names, mat = gc.shuffled(gc.row_median_planted(n))
    more, rest = _planted_matrix(n, with_nan=False)
    _check(monkeypatch, name, np.vstack([mat, rest]), names=names + more)


@pytest.mark.parametrize("name", ["sum128", "sum300"])
def test_run_sums_in_numpys_order(name, monkeypatch):
    """Every count 1..128 through gv_numpy_sum; counts up to 300 through numpy_sum's recursion, on the plan that takes the
    round-1 kernels by itself.  Windows +-2^e * m: another order of the additions changes the bits."""
    plan, runs = _plan(name)
    fused, _, _ = _launch_shape(plan, runs)
    if name == "sum128":
        assert fused and set(runs["count"]) >= set(range(1, 129))
    else:
        assert not fused and runs["count"].max() == 300 and runs["genes"].sum() > 1024
    win = gc.order_sensitive(6, plan.n_windows, seed=31)
    seq = np.array([gc.sequential_run_values(runs, row) for row in win[:2]])
    num = np.array([go.run_values(runs, row) for row in win[:2]])
    assert 3 * (seq != num).sum() >= seq.size
    _check(monkeypatch, name, win)
    _check(monkeypatch, name, gc.dyadic(5, plan.n_windows, seed=32), thr=np.array([0.125, 1.0]), chunksize=3)


@pytest.mark.parametrize("name", ["odd", "even"])
@pytest.mark.parametrize("win_layout", ["contiguous", "even_stride", "one_past_16"])
@pytest.mark.parametrize("out_layout", ["own", "view", "even_view"])
def test_window_and_output_layouts(name, win_layout, out_layout, monkeypatch):
    """16-byte window loads on / off (odd row stride; a base one double past a 16-byte boundary), W odd with the last
    window stored by thread 0; 16-byte stores off (``view``: an odd row stride and an 8-byte-only aligned base; ``own``
    with an odd n_cols: the odd stride of the contiguous layer) and on (``own`` with an even n_cols; ``even_view``: the
    first n_cols columns of a 16-byte aligned buffer of even row stride -- for the odd n_cols the ONLY layout in which
    the 16-byte path stores a row's last column alone, from the padded table word).  The columns around a view stay
    untouched."""
    import torch

    from infercnvpy_amd import _engine

    plan, runs = _plan(name)
    W, n_cols = plan.n_windows, plan.n_cols_all
    assert W % 2 == n_cols % 2 == (name == "odd") and (runs["count"] == 1).all() and (runs["genes"] == 1).all()
    names, mat = _planted_matrix(W)
    rows = mat.shape[0]
    want = go.gene_layer(runs, mat, n_cols)
    if win_layout == "contiguous":        # odd W: odd stride, 8-byte loads; even W: 16-byte loads
        d_win = _device(mat)
    else:
        ld = W + 2 + W % 2                # even
        buf = torch.full((rows, ld), float("nan"), dtype=torch.float64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        d_win = buf[:, :W] if win_layout == "even_stride" else buf[:, 1:1 + W]
        d_win.copy_(_device(mat))
        assert d_win.stride(0) % 2 == 0 and d_win.data_ptr() % 16 == (0 if win_layout == "even_stride" else 8)

    def call():
        if out_layout == "own":
            return _engine.gene_values_from_windows(plan, d_win, n_vars=n_cols)
        if out_layout == "even_view":
            wide = torch.full((rows, n_cols + 1 + (n_cols + 1) % 2), 7.0, dtype=torch.float64, device="cuda")
            out = _engine.gene_values_from_windows(plan, d_win, out=wide[:, :n_cols])
            assert out.stride(0) % 2 == 0 and out.data_ptr() % 16 == 0 and wide.shape[1] - n_cols in (1, 2)
            assert float(wide[:, n_cols:].min()) == 7.0 == float(wide[:, n_cols:].max())  # the spare column(s)
            return out
        ld = n_cols + 3 if n_cols % 2 == 0 else n_cols + 4  # odd
        wide = torch.full((rows, ld), 7.0, dtype=torch.float64, device="cuda")
        out = _engine.gene_values_from_windows(plan, d_win, out=wide[:, 1:1 + n_cols])
        assert out.stride(0) % 2 == 1 and out.data_ptr() % 16 == 8
        assert float(wide[:, 0].min()) == 7.0 == float(wide[:, 0].max())
        assert float(wide[:, 1 + n_cols:].min()) == 7.0 == float(wide[:, 1 + n_cols:].max())  # nothing outside the view
        return out

    got = _both_routes(monkeypatch, call)
    for route in ROUTES:
        go.same_bytes(got[route], want)


@pytest.mark.parametrize("win16,vec2", [(True, True), (True, False), (False, True), (False, False)])
def test_more_rows_than_workgroups(win16, vec2, monkeypatch):
    """8 x CUs + 77 rows: every workgroup of the persistent launch (at most 4 x CUs) takes two cells and some three, the
    later ones from the register prefetch and with the scratch over the previous cell's windows.  Row i = planted pattern
    i % n_patterns shifted by an exact constant of its own: nothing left over from another cell gives its answer.
    The next cell's prefetch is issued at one place with 16-byte stores (``vec2``: the contiguous even layer, or an
    aligned even-stride view for the odd n_cols) and at another without (an odd-stride view / the contiguous odd layer);
    without 16-byte window loads nothing is prefetched."""
    import torch

    from infercnvpy_amd import _engine

    name = "even" if win16 else "odd"
    plan, runs = _plan(name)
    W, n_cols = plan.n_windows, plan.n_cols_all
    assert (runs["count"] == 1).all() and (runs["genes"] == 1).all() and _launch_shape(plan, runs)[0]
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = 8 * cu + 77
    pats = gc.planted(W)
    keep = [k for k in pats if not k.startswith(("adjacent", "nested"))]  # multiples of 2^-20: the shift is exact
    _, base = gc.shuffled({k: pats[k] for k in keep})
    assert (base == np.round(base / gc.U) * gc.U).all() and len(keep) >= 10
    assert (4 * cu) % len(keep) != 0  # a workgroup's next cell is another pattern
    idx = np.arange(n)
    shift = (idx // len(keep) + 1) * 2.0 ** -7 * np.where(idx % 2, 1.0, -1.0)
    win = base[idx % len(keep)] + shift[:, None]
    assert (win - shift[:, None] == base[idx % len(keep)]).all()
    thr = np.array([0.5, 0.0, 2.0 ** -10, 1.0, 0.25])
    chunksize = n // 5 + 1
    want = go.gene_layer(runs, win, n_cols, thr=thr, chunksize=chunksize)
    d_win, d_thr = _device(win), _device(thr)
    assert (d_win.stride(0) % 2 == 0 and d_win.data_ptr() % 16 == 0) == win16

    def call():
        if vec2 == (n_cols % 2 == 0):  # the contiguous layer: 16-byte stores exactly where n_cols is even
            out = _engine.gene_values_from_windows(plan, d_win, thr=d_thr, chunksize=chunksize, n_vars=n_cols)
        elif vec2:                     # odd n_cols, aligned view of even stride
            wide = torch.full((n, n_cols + 1), 7.0, dtype=torch.float64, device="cuda")
            out = _engine.gene_values_from_windows(plan, d_win, thr=d_thr, chunksize=chunksize, out=wide[:, :n_cols])
            assert float(wide[:, n_cols:].min()) == 7.0 == float(wide[:, n_cols:].max())
        else:                          # even n_cols, view of odd stride from an 8-byte-only aligned base
            wide = torch.full((n, n_cols + 3), 7.0, dtype=torch.float64, device="cuda")
            out = _engine.gene_values_from_windows(plan, d_win, thr=d_thr, chunksize=chunksize, out=wide[:, 1:1 + n_cols])
            assert float(wide[:, 0].min()) == 7.0 == float(wide[:, 0].max())
            assert float(wide[:, 1 + n_cols:].min()) == 7.0 == float(wide[:, 1 + n_cols:].max())
        assert (out.stride(0) % 2 == 0 and out.data_ptr() % 16 == 0) == vec2
        return out

    got = _both_routes(monkeypatch, call)
    for route in ROUTES:
        go.same_bytes(got[route], want)


@pytest.mark.parametrize("name", ["odd", "even"])
def test_noise_filter_at_the_threshold(name, monkeypatch):
    """The strict < at |v| == thr, one ulp inside and outside, under three chunks of a size that does not divide the
    rows, with row_phase 0 and a row_phase that moves the chunk boundaries; and without thresholds."""
    plan, runs = _plan(name)
    rows, chunksize = 20, 8
    assert (runs["count"] == 1).all() and (runs["genes"] == 1).all()
    win = gc.filter_rows(rows, plan.n_windows)
    assert rows % chunksize and -(-rows // chunksize) == len(gc.FILTER_THR) == -(-(rows + 3) // chunksize)
    a = _check(monkeypatch, name, win, thr=gc.FILTER_THR, chunksize=chunksize, row_phase=0)
    b = _check(monkeypatch, name, win, thr=gc.FILTER_THR, chunksize=chunksize, row_phase=3)
    c = _check(monkeypatch, name, win)
    assert not np.array_equal(np.nan_to_num(a), np.nan_to_num(b)) and (np.nan_to_num(c) != 0).sum() > (np.nan_to_num(a) != 0).sum()
    for i in range(rows):
        t = gc.FILTER_THR[i // chunksize]
        assert (np.abs(a[i]) == t).sum() >= 2 and (np.abs(c[i]) == t).sum() == (np.abs(a[i]) == t).sum()

"""Which smoothing kernel a call takes, and that the choice changes no bit (``-m gpu``).

The library picks the kernel of a call in one place (``pick_route`` in ``csrc/icv_api.hip``) from the plan's geometry,
the matrix, the developer knobs and from what the caller wants back: per-cell moments (``cell_stats=True``), only the
thresholds (``cell_stats=False``: the moments are formed per chunk inside the kernels that can) or the float64 windows as
well (``windows=True``).  Every case below is a 70-row matrix on a geometry of
``test_fast_and_generic_kernels_are_bit_identical`` (plus the float64 gene set of
``test_gene_sets_larger_than_lds_split_by_chromosome_group`` for the chromosome-group path), run in those three modes:

(a) ``plan.last_kernel()`` is the kind the table names for the mode.  The kinds were observed on the commit before the
    routing was gathered into ``pick_route`` and copied here; together they reach every ``ICV_KERNEL_*`` value.  A dense
    geometry outside k_smooth_x16 and the prepared-entry CSR kernel write no windows: with ``windows=True`` those calls go
    to the generic kernel.
(b) without a threshold, ``out`` and ``cell_median`` are the same bits in all three modes;
(c) with it, the thresholds from the per-chunk moments agree with those from the per-cell moments to the tolerance of
    ``test_fast_and_generic_kernels_are_bit_identical`` for that comparison (1e-12; 1e-9 for k_smooth_se).

70 rows are no multiple of any chunk size used, and two cases start inside a chunk (``row_phase > 0``): a wrong count of
partial-moment slots or a wrong chunk index shows in the thresholds.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import cases

pytestmark = pytest.mark.gpu

N_ROWS = 70
KNOBS = ("ICV_FORCE_GENERIC", "ICV_NO_X16", "ICV_NO_SD")
SMALL = (230, 110, 101, 100, 99, 57, 140)
ODD = (600, 260, 251, 250, 249)
F64_SPLIT = (2600, 2400, 2300, 2200, 2100, 2000, 1900, 1800, 1700, 1600, 1500, 1400, 900, 800)  # 25 200 genes
G20K = tuple(cases.GENES_PER_CHROM_20K)

# name: (genes per chromosome, window, step, dtype, format, knobs, chunksize, row_phase,
#        kinds with cell_stats=True / cell_stats=False / windows=True, threshold tolerance)
CASES = {
    "x16_w100": (G20K, 100, 10, "f32", "dense", (), 32, 0, ("X16", "X16", "X16"), 1e-12),
    "x16_w250_phase": (G20K, 250, 10, "f32", "dense", (), 16, 5, ("X16", "X16", "X16"), 1e-12),
    "ws_no_windows": (G20K, 100, 10, "f32", "dense", ("ICV_NO_X16",), 32, 0, ("WS", "WS", "GENERIC"), 1e-12),
    "small_dense": (SMALL, 100, 10, "f32", "dense", (), 32, 0, ("GENERIC", "GENERIC", "GENERIC"), 1e-12),
    "odd_dense": (ODD, 20, 4, "f32", "dense", (), 32, 0, ("GENERIC", "GENERIC", "GENERIC"), 1e-12),
    "generic": (G20K, 100, 10, "f32", "dense", ("ICV_FORCE_GENERIC",), 32, 0, ("GENERIC", "GENERIC", "GENERIC"), 1e-12),
    "sd_w100": (G20K, 100, 10, "f32", "csr", (), 32, 0, ("SD", "SD", "SD"), 1e-9),
    "sd_w250_phase": (G20K, 250, 10, "f32", "csr", (), 16, 3, ("SD", "SD", "SD"), 1e-9),
    "ws_csr_no_windows": (G20K, 100, 10, "f32", "csr", ("ICV_NO_SD",), 32, 0, ("WS_CSR", "WS_CSR", "GENERIC"), 1e-12),
    "split_f64": (F64_SPLIT, 100, 10, "f64", "dense", (), 32, 0, ("SPLIT", "SPLIT", "SPLIT"), 1e-12),
}
MODES = (dict(cell_stats=True), dict(cell_stats=False), dict(cell_stats=False, windows=True))


@functools.lru_cache(maxsize=None)
def _geometry(genes, window, step, dtype):
    """(plan, host matrix, device reference) of one geometry: shared by the cases on it and left unchanged."""
    import torch

    from infercnvpy_amd._plan import GenePlan

    v = cases.synthetic_var(list(genes), extra=(("chrX", 31), (None, 3)))
    n_genes = len(v["names"]) - len(v["names"]) % 4
    plan = GenePlan(v["chromosome"][:n_genes], v["start"][:n_genes], window_size=window, step=step)
    np_dtype = np.float32 if dtype == "f32" else np.float64
    X = cases.synthetic_expr(N_ROWS, n_genes, seed=21, dtype=np_dtype)
    ref = X[7:].mean(axis=0, dtype=np.float64).astype(np_dtype)
    X[5] = ref  # centred row is all zero: every window ties at the median (handed back by the histogram kernels)
    X[6, 17] = np.nan
    return plan, X, torch.from_numpy(ref).cuda()


def _same_bits(a, b):
    import torch

    return torch.equal(torch.nan_to_num(a, nan=123.0), torch.nan_to_num(b, nan=123.0))


@pytest.mark.parametrize("name", list(CASES))
def test_route_of_every_mode_and_same_bits_across_modes(name, monkeypatch):
    import torch

    from infercnvpy_amd import _engine, _lib

    genes, window, step, dtype, fmt, knobs, chunksize, row_phase, kinds, tol = CASES[name]
    plan, X, ref = _geometry(genes, window, step, dtype)
    dm = _engine.to_device_matrix(sp.csr_matrix(X) if fmt == "csr" else X)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k in knobs:
        monkeypatch.setenv(k, "1")
    _lib.load().icv_developer_knobs_reload()

    def run(mode, dyn):
        res = _engine.run_hot_path(plan, dm, ref, dynamic_threshold=dyn, chunksize=chunksize, row_phase=row_phase, **mode)
        torch.cuda.synchronize()
        return res, plan.last_kernel()

    want = tuple(getattr(_lib, "ICV_KERNEL_" + k) for k in kinds)
    plain = [run(mode, None) for mode in MODES]
    with_thr = [run(mode, 1.5) for mode in MODES[:2]]
    got = tuple(k for _, k in plain)
    print(f"{name}: kinds {got} without a threshold, {tuple(k for _, k in with_thr)} with one")
    assert got == want and tuple(k for _, k in with_thr) == want[:2]
    base = plain[0][0]
    assert torch.isnan(base.out[6]).all() and not torch.isnan(base.out[:6]).any() and (base.out[5] == 0).all()
    for (res, _), mode in zip(plain[1:], MODES[1:]):
        assert _same_bits(res.out, base.out), (name, mode)
        assert _same_bits(res.cell_median, base.cell_median), (name, mode)
    assert plain[2][0].windows.shape == (N_ROWS, plan.n_windows)
    (full, _), (lean, _) = with_thr
    assert full.cell_stats is not None and lean.cell_stats is None
    assert lean.thr.shape == full.thr.shape == (-(-(N_ROWS + row_phase) // chunksize),)
    assert not torch.isnan(full.thr[1:]).any()  # (chunk 0 holds the NaN cell)
    torch.testing.assert_close(lean.thr, full.thr, rtol=tol, atol=tol, equal_nan=True)

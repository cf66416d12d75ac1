"""GPU tests (``-m gpu``) of the dense ``k_colchain`` split in 64-byte units (``ChainLaunch.dense_grid`` /
``chain_tile_units``, ``csrc/icv_kernel_chain.hpp``): at any width every column is added by exactly one workgroup, as
ONE ascending chain in the matrix dtype.  The accumulators are compared ``array_equal`` with numpy adding the rows one
after the other (``acc = acc + x[r]`` in float32 / float64 is numpy's own ``np.mean`` order for a C-contiguous matrix).

Widths: 1 and 7 columns (one unit, one workgroup), 625 / 626 (float32: 40 units, the first partial), 20 000 (the
headline's 1 250 units over the CUs: tiles of 4 and 5 units), 40 001 (more cache lines than four per CU: half the LDS,
tiles of whole lines) and odd float64 widths; with and without a row list, starting from zero and continuing a chain."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _numpy_chain(X, rows, acc0):
    acc = acc0.copy()
    for r in rows:
        acc = acc + X[r]  # elementwise in the matrix dtype: one rounding per add, rows ascending
    return acc


def _expr(n, g, seed, dtype):
    rs = np.random.RandomState(seed)
    X = (rs.gamma(0.3, 1.0, size=(n, g)) * rs.choice([1.0, 1e-3, 1e3], size=(1, g))).astype(dtype)
    X[X < 0.2] = 0
    return X


def _gpu_chain(X, rows, acc0):
    from infercnvpy_amd import _engine

    torch = _engine._torch()
    dm = _engine.to_device_matrix(X)
    acc = torch.from_numpy(acc0.copy()).to("cuda")
    acc = _engine.column_chain(dm, acc, rows, X.shape[0])
    torch.cuda.synchronize()
    return acc.cpu().numpy()


CASES = [
    (np.float32, 1), (np.float32, 7), (np.float32, 625), (np.float32, 626), (np.float32, 20000), (np.float32, 40001),
    (np.float64, 1), (np.float64, 313), (np.float64, 4999), (np.float64, 10001),
]


@pytest.mark.parametrize("dtype,g", CASES, ids=[f"{np.dtype(d).name}-{g}" for d, g in CASES])
@pytest.mark.parametrize("with_rows", [False, True], ids=["all_rows", "row_list"])
def test_dense_chain_split_matches_numpy_row_by_row(dtype, g, with_rows):
    n = 517 if g <= 20000 else 131  # (not a multiple of any round's rows: the last round is partial)
    X = _expr(n, g, seed=g + 7 * with_rows, dtype=dtype)
    rows = np.sort(np.random.RandomState(g).choice(n, size=n // 3, replace=False)) if with_rows else None
    if with_rows:
        rows[-1] = n - 1  # the list ends with the buffer's last row (the guarded tail when the row is not 16-byte padded)
    acc0 = np.random.RandomState(g + 1).standard_normal(g).astype(dtype)  # a chain continued, not started
    got = _gpu_chain(X, rows, acc0)
    exp = _numpy_chain(X, range(n) if rows is None else rows, acc0)
    assert got.dtype == exp.dtype
    assert np.array_equal(got, exp), (g, int(np.sum(got != exp)), np.nonzero(got != exp)[0][:10])


@pytest.mark.parametrize("cols", [(1, 20000), (3, 630), (16, 17)])
def test_dense_chain_split_on_a_column_range(cols):
    """Ranks pipelining over column groups (``dist.py``) chain a column range of the full rows."""
    from infercnvpy_amd import _engine

    torch = _engine._torch()
    n, g = 301, 20000
    X = _expr(n, g, seed=11, dtype=np.float32)
    dm = _engine.to_device_matrix(X)
    acc = torch.zeros(g, dtype=torch.float32, device="cuda")
    acc = _engine.column_chain(dm, acc, None, n, cols=cols)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    c0, c1 = cols
    exp = np.zeros(g, np.float32)
    exp[c0:c1] = _numpy_chain(X[:, c0:c1], range(n), np.zeros(c1 - c0, np.float32))
    assert np.array_equal(got, exp)

"""CPU tests of bench.py's --dump-outputs writer: which rows it keeps, the size budget, the file types, and that the
same X_cnv gives the same files (two builds of the project are compared through them)."""
import os

import numpy as np
import scipy.sparse as sp
import torch

import bench


class _Packed:
    """The part of PackedCsr that dump_outputs reads."""

    def __init__(self, m):
        self.m = m

    def to_scipy(self):
        return self.m


def _x_cnv(n, w):
    m = sp.random(n, w, density=0.05, format="csr", random_state=2, dtype=np.float64)
    m.data = (m.data - 0.5).astype(np.float32).astype(np.float64)  # float32 values widened, as X_cnv's
    return m


def _load(d):
    files = sorted(os.listdir(d))
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


def test_dump_of_a_packed_csr(tmp_path):
    n, w = 3000, 3000  # 3000 rows of 3000 float64 windows = 72 MB: more than the budget of the dense rows
    m = _x_cnv(n, w)
    bench.dump_outputs(str(tmp_path / "a"), _Packed(m), {"chr1": 0, "chr2": 17})
    a = _load(tmp_path / "a")
    idx = a["x_cnv_row_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_ROWS_BYTES // (8 * w) < n
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    np.testing.assert_array_equal(a["x_cnv_rows"], m[idx].toarray())
    np.testing.assert_array_equal(a["x_cnv_row_sum"], np.asarray(m.sum(axis=1)).ravel())
    np.testing.assert_array_equal(a["x_cnv_row_nnz"], np.diff(m.indptr))
    np.testing.assert_array_equal(a["chr_pos"], [0, 17])
    assert "x_cnv_row_stats_index" not in a  # every row's sum and count

    bench.dump_outputs(str(tmp_path / "b"), _Packed(m.copy()), {"chr1": 0, "chr2": 17})
    b = _load(tmp_path / "b")
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_dump_of_a_dense_result_and_of_ranks(tmp_path):
    n, w = 3000, 3000
    m = _x_cnv(n, w)
    dense = torch.from_numpy(m.toarray().astype(np.float32))
    bench.dump_outputs(str(tmp_path), dense, {"chr1": 0}, suffix=".rank1", share=2)
    d = _load(tmp_path)
    assert all(k.endswith(".rank1") for k in d)
    idx = d["x_cnv_row_index.rank1"].astype(np.int64)
    assert len(idx) == bench.DUMP_ROWS_BYTES // 2 // (8 * w)
    np.testing.assert_array_equal(d["x_cnv_rows.rank1"], m[idx].toarray())
    np.testing.assert_allclose(d["x_cnv_row_sum.rank1"], np.asarray(m.sum(axis=1)).ravel(), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(d["x_cnv_row_nnz.rank1"], np.diff(m.indptr))


def test_dump_of_many_rows_samples_the_row_digests(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROW_STATS", 500)
    m = _x_cnv(2000, 40)
    bench.dump_outputs(str(tmp_path), _Packed(m), {"chr1": 0})
    d = _load(tmp_path)
    assert d["x_cnv_row_index"].shape == (2000,)  # the dense rows all fit
    si = d["x_cnv_row_stats_index"].astype(np.int64)
    assert len(si) == 500 and np.all(np.diff(si) > 0)
    np.testing.assert_array_equal(d["x_cnv_row_sum"], np.asarray(m.sum(axis=1)).ravel()[si])
    np.testing.assert_array_equal(d["x_cnv_row_nnz"], np.diff(m.indptr)[si])

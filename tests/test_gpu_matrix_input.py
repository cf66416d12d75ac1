"""GPU tests (``-m gpu``): ``_engine.matrix_input``, the one intake of ``obsm["X_cnv"]`` for tl.pca, the HMM functions and
tl.cnv_pseudobulk.  Every storage it takes gives the matrix's values and the documented dtype; what it reads back depends
on the caller alone; and every consumer reads the same values from the four forms of one matrix, which also takes every
entry point that picks a kernel by (dtype, format) through all of its instantiations."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

# 5 x 7, an all-zero second and last row; the CSR forms store the 0.0 at (2, 3)
X = np.asarray([[0.5, 0, 0, -1.25, 0, 0, 2.0],
                [0, 0, 0, 0, 0, 0, 0],
                [0, 3.0, 0, 0.0, 0, -0.75, 0],
                [1.5, 0, 0, 0, 0, 0, -4.0],
                [0, 0, 0, 0, 0, 0, 0]], dtype=np.float64)
INDPTR = np.asarray([0, 3, 3, 6, 8, 8], dtype=np.int64)
INDICES = np.asarray([0, 3, 6, 1, 3, 5, 0, 6], dtype=np.int32)
DATA = np.asarray([0.5, -1.25, 2.0, 3.0, 0.0, -0.75, 1.5, -4.0], dtype=np.float64)


def _canonical(dtype):
    m = sp.csr_matrix((DATA.astype(dtype), INDICES.copy(), INDPTR.copy()), shape=X.shape)
    assert m.nnz == 8 and m.has_canonical_format
    return m


def _unsorted_with_a_duplicate():
    # row 0 as (6: 2.0), (0: 0.25), (3: -1.25), (0: 0.25); the other rows as above
    m = sp.csr_matrix((np.concatenate([[2.0, 0.25, -1.25, 0.25], DATA[3:]]), np.concatenate([[6, 0, 3, 0], INDICES[3:]]),
                       INDPTR + np.asarray([0, 1, 1, 1, 1, 1])), shape=X.shape)
    assert m.nnz == 9 and not m.has_canonical_format
    return m


def _read_only_fortran():
    a = np.asfortranarray(X)
    a.setflags(write=False)
    assert not a.flags.c_contiguous
    return a


def _column_sliced_view():
    import torch

    wide = np.full((5, 9), 77.0, dtype=np.float32)
    wide[:, 1:8] = X
    view = torch.from_numpy(wide).cuda()[:, 1:8]
    assert view.stride(0) == 9
    return view


def _packed_with_spare_capacity():
    import torch

    from infercnvpy_amd import _engine

    spare = 5  # entries behind nnz that belong to no row
    return _engine.PackedCsr(torch.from_numpy(INDPTR).cuda(),
                             torch.from_numpy(np.concatenate([INDICES, np.full(spare, 6, dtype=np.int32)])).cuda(),
                             torch.from_numpy(np.concatenate([DATA, np.full(spare, 1e30)])).cuda(), 7)


def _cuda_int64():
    import torch

    return torch.from_numpy((X * 4).astype(np.int64)).cuda()


STORAGES = {  # name: (() -> input, the values it holds, dtype of the DeviceMatrix, its format)
    "canonical CSR float32": (lambda: _canonical(np.float32), X, "float32", "csr"),
    "CSC float64": (lambda: _canonical(np.float64).tocsc(), X, "float64", "csr"),
    "CSR unsorted with a duplicate": (_unsorted_with_a_duplicate, X, "float64", "csr"),
    "host dense int32": (lambda: (X * 4).astype(np.int32), X * 4, "float64", "dense"),
    "host dense float64 read-only Fortran": (_read_only_fortran, X, "float64", "dense"),
    "CUDA float32 column-sliced view": (_column_sliced_view, X, "float32", "dense"),
    "CUDA int64": (_cuda_int64, X * 4, "float64", "dense"),
    "PackedCsr with spare capacity": (_packed_with_spare_capacity, X, "float64", "csr"),
}


def _to_host(m):
    """The matrix a DeviceMatrix (or the host array of a slab-wise caller) holds, rebuilt on the host from its tensors."""
    from infercnvpy_amd import _lib

    if isinstance(m, np.ndarray):
        return m
    if m.format == _lib.ICV_DENSE:
        return m.dense.cpu().numpy()
    indptr = m.indptr.cpu().numpy()
    nnz = int(indptr[-1])
    csr = sp.csr_matrix((m.data.cpu().numpy()[:nnz], m.indices.cpu().numpy()[:nnz], indptr), shape=m.shape)
    assert csr.has_canonical_format or nnz == 0
    return csr.toarray()


@pytest.mark.parametrize("slabs", [False, True])
@pytest.mark.parametrize("name", list(STORAGES))
def test_every_storage_gives_the_matrixs_values_and_the_documented_dtype(name, slabs):
    import torch

    from infercnvpy_amd import _engine, _lib

    make, values, dtype, fmt = STORAGES[name]
    m = _engine.matrix_input(make(), "tl.somebody", slabs=slabs)
    if slabs and name.startswith("host dense"):  # left on the host for the slab-wise upload
        assert isinstance(m, np.ndarray) and m.flags.c_contiguous and str(m.dtype) == dtype
    else:
        assert isinstance(m, _engine.DeviceMatrix) and m.dtype == getattr(torch, dtype)
        assert m.format == (_lib.ICV_CSR if fmt == "csr" else _lib.ICV_DENSE)
        if fmt == "dense":
            assert m.dense.is_contiguous() and m.c_struct().ld == 7
    got = _to_host(m)
    assert got.shape == (5, 7) and str(got.dtype) == dtype and np.array_equal(got, values)
    assert not got[1].any() and not got[4].any()


def test_pca_input_keeps_its_fields():
    from infercnvpy_amd import _engine

    for name, (make, values, dtype, _) in STORAGES.items():
        inp = _engine._PcaInput(make())
        assert inp.shape == (5, 7) and (inp.dm is None) == name.startswith("host dense"), name
        assert (inp.host_dense is None) == (inp.dm is not None), name
        assert inp.f32_exact == (dtype == "float32" or name.startswith("PackedCsr")), name
        got = np.concatenate([_to_host(dm)[r0:r0 + m.n_rows] if inp.dm is not None else _to_host(dm)
                              for r0, dm, m in inp.slabs(2)])
        assert np.array_equal(got, values), name


@pytest.mark.parametrize("make", [lambda: np.ones(4), lambda: np.ones((2, 3, 4)), lambda: __import__("torch").ones(4).cuda(),
                                  lambda: __import__("torch").ones((2, 3, 4), device="cuda")],
                         ids=["host 1-D", "host 3-D", "CUDA 1-D", "CUDA 3-D"])
def test_an_input_that_is_not_2_d_raises_with_the_callers_name(make):
    from infercnvpy_amd import _engine

    for who, slabs in (("tl.somebody", False), ("tl.pca", True)):
        with pytest.raises(ValueError) as info:
            _engine.matrix_input(make(), who, slabs=slabs)
        assert info.value.args[0] == f"{who}: X must be 2-D"
    with pytest.raises(ValueError) as info:
        _engine._PcaInput(make())
    assert info.value.args[0] == "tl.pca: X must be 2-D"


def test_a_packed_csr_is_read_back_only_for_the_caller_that_slices_rows(monkeypatch):
    import torch

    from infercnvpy_amd import _engine

    packed = _packed_with_spare_capacity()
    fetched = []
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (fetched.append(self.data_ptr()), to_host(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a scalar was read back"))
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: pytest.fail("a tensor was read back"))
    dm = _engine.matrix_input(packed, "tl.cnv_states")  # the HMM functions and tl.cnv_pseudobulk: no slicing
    assert fetched == [] and not dm.indptr_host.any()
    m = dm.c_struct()
    assert (m.n_rows, m.csr_begin, m.csr_end) == (5, 0, 0)
    sliced = _engine.matrix_input(packed, "tl.pca", slabs=True)  # tl.pca: the row pointers of its slabs
    assert fetched == [packed.indptr.data_ptr()] and np.array_equal(sliced.indptr_host, INDPTR)
    m = sliced.c_struct(2, 4)
    assert (m.n_rows, m.csr_begin, m.csr_end) == (2, 3, 8)
    for d in (dm, sliced):  # both read the PackedCsr where it lies
        assert d.data.data_ptr() == packed.data.data_ptr() and d.indices.data_ptr() == packed.indices.data_ptr()


# ---- every consumer reads the same values from the four forms of one matrix ------------------------------------------------
N, W = 3, 65  # one window more than a wavefront
CHR_POS = {"chr1": 0, "chr2": 33}


def _values():
    rng = np.random.RandomState(11)
    x = (rng.standard_normal((N, W)) * 0.1).astype(np.float32)
    x[rng.uniform(size=(N, W)) < 0.4] = 0
    x[0, 5:20] += np.float32(0.5)  # a gain and a loss, so that the calls are not all neutral
    x[2, 40:60] -= np.float32(0.5)
    x[1] = 0  # a row of no stored entries
    return x


def _forms():
    x = _values()
    return {"csr_float32": sp.csr_matrix(x), "csr_float64": sp.csr_matrix(x.astype(np.float64)), "dense_float32": x,
            "dense_float64": x.astype(np.float64)}


def _adata(x):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((N, 2), dtype=np.float32), obs=pd.DataFrame({"clone": ["a"] * N}))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(CHR_POS)}
    return ad


def _gram_direct(dm, panel_float32):
    """icv_gram_f64 on one DeviceMatrix with the panel type of the caller's choice (_engine.gram picks it from the matrix)."""
    import torch

    from infercnvpy_amd import _engine, _lib

    ld = -(-W // 64) * 64
    g = torch.empty((W, W), dtype=torch.float64, device="cuda")
    panel = torch.empty(32 * ld, dtype=torch.float32 if panel_float32 else torch.float64, device="cuda")
    m = dm.c_struct()
    _lib.check(_lib.load().icv_gram_f64(ctypes.byref(m), _lib.ICV_F32 if panel_float32 else _lib.ICV_F64, _engine._ptr(panel),
                                        ld, _engine._ptr(g), W, 0, _engine._stream_ptr(torch)))
    return g.cpu().numpy()


@pytest.fixture(scope="module")
def consumed():
    """What every consumer gives on each of the four forms, as bytes or exact floats."""
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    v = np.linalg.qr(np.random.RandomState(3).standard_normal((W, 3)))[0]
    shift = np.asarray([0.25, -0.5, 0.125])
    out = {}
    for name, x in _forms().items():
        states, fraction = cnv.tl.cnv_states(_adata(x), inplace=False)
        loss, neutral, gain = cnv.tl.cnv_posteriors(_adata(x), inplace=False, all_states=True)
        fit = cnv.tl.cnv_states_fit(_adata(x), inplace=False, max_iter=2)
        clones = cnv.tl.cnv_pseudobulk(_adata(x), "clone")
        dm = _engine.matrix_input(x, "test")
        out[name] = {
            "states": states.tobytes(), "fraction": fraction.tobytes(), "neutral": neutral.tobytes(),
            "loss": loss.tobytes(), "gain": gain.tobytes(), "fit": repr(sorted(fit.items())),
            "mean": clones.obsm["X_cnv"].tobytes(), "stored": clones.obsm["X_cnv_fraction"].tobytes(),
            "gram": _engine.gram(x, zero_center=True)[0].tobytes(),
            "gram_f32_panel": _gram_direct(dm, True).tobytes(), "gram_f64_panel": _gram_direct(dm, False).tobytes(),
            "project_f32": _engine.project(x, v, shift, np.float32).tobytes(),
            "project_f64": _engine.project(x, v, shift, np.float64).tobytes(),
        }
        assert np.any(states != 0) and states.dtype == np.int8 and neutral.dtype == np.float64
    return out


@pytest.mark.parametrize("what", ["states", "fraction", "neutral", "loss", "gain", "fit", "mean", "stored", "gram",
                                  "gram_f32_panel", "gram_f64_panel", "project_f32", "project_f64"])
def test_the_four_forms_of_one_matrix_give_the_same_bytes(consumed, what):
    """float32 values in float32 or float64, CSR or dense: tl.cnv_states, tl.cnv_posteriors, tl.cnv_states_fit (DESIGN.md
    4.13 rule 1: stored values as float64, a dense row's zeros add +0.0), tl.cnv_pseudobulk (4.17) and tl.pca's Gram and
    projection (4.8: a float32 panel holds float32 numbers exactly; sums in stored-entry order) do not see the storage."""
    first = consumed["csr_float32"][what]
    for name, got in consumed.items():
        assert got[what] == first, (what, name)


def test_the_gram_does_not_depend_on_the_panel_type_for_float32_values(consumed):
    for name, got in consumed.items():
        assert got["gram_f32_panel"] == got["gram_f64_panel"] == got["gram"], name


def test_the_consumers_results_are_the_values_own():
    """The common bytes are not common garbage: the Gram against numpy, the pseudobulk mean against the column means."""
    from infercnvpy_amd import _engine

    x = _values().astype(np.float64)
    g, _ = _engine.gram(x)
    assert np.array_equal(g, g.T) and np.allclose(g, x.T @ x, rtol=1e-13, atol=1e-15)
    import infercnvpy_amd as cnv

    clones = cnv.tl.cnv_pseudobulk(_adata(sp.csr_matrix(x)), "clone")
    assert np.allclose(clones.obsm["X_cnv"][0], x.mean(axis=0), rtol=0, atol=2.0 ** -40)
    assert np.array_equal(clones.obsm["X_cnv_fraction"][0], (x != 0).mean(axis=0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_csr_entry_points_of_tl_cnv_score_and_tl_ithcna_take_both_value_types(dtype):
    """icv_csr_row_abs_sum (host CSR and PackedCsr) and icv_csr_densify on float32 and float64 stored values."""
    import torch

    from infercnvpy_amd import _engine

    x = _values()
    csr = sp.csr_matrix(x.astype(dtype))
    packed = _engine.PackedCsr(torch.from_numpy(csr.indptr.astype(np.int64)).cuda(), torch.from_numpy(csr.indices).cuda(),
                               torch.from_numpy(csr.data).cuda(), W)
    want = np.abs(x.astype(np.float64)).sum(axis=1)
    for inp in (csr, packed):
        got = _engine.csr_row_abs_sum(inp).cpu().numpy()
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-14, atol=0) and got[1] == 0.0
    assert np.array_equal(_engine.csr_row_abs_sum(csr).cpu().numpy(), _engine.csr_row_abs_sum(packed).cpu().numpy())
    tile = packed.dense_rows([2, 0]).cpu().numpy()
    assert tile.dtype == np.float32 and np.array_equal(tile, x[[2, 0]])

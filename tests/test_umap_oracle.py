"""The numpy oracle of tl.umap keeps its own invariants; tl.umap / pl.umap argument errors and the two
C-ABI symbols, as far as they need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _leiden_oracle as lo
import _umap_oracle as uo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = uo.A_DEFAULT, uo.B_DEFAULT
KW = dict(n_epochs=50, a=A, b=B)


@pytest.fixture(scope="module")
def mix():
    g = lo.mixture_graph(300, 0)
    return g, uo.Graph(g)


def test_curve_fit_of_the_defaults():
    a, b = uo.find_ab(1.0, 0.5)
    assert abs(a - 0.5830) < 1e-3 and abs(b - 1.3342) < 1e-3
    assert abs(a - A) < 1e-6 and abs(b - B) < 1e-6
    from infercnvpy_amd.tl._umap import find_ab_params

    assert find_ab_params(1.0, 0.5) == (a, b)


def test_epoch_zero_is_the_identity(mix):
    _, og = mix
    y = uo.random_init(og.n, 2, 0)
    new, m = uo.epoch(og, y, 0, **KW)
    assert new.tobytes() == y.tobytes() and not m.any()


def test_the_sum_does_not_depend_on_the_order(mix):
    _, og = mix
    y = uo.random_init(og.n, 3, 1)
    ref, m = uo.epoch(og, y, 7, seed=1, **KW)
    assert m.sum() > 0 and (m % 6 == 0).all() and not np.array_equal(ref, y)
    rng = np.random.default_rng(0)
    for _ in range(3):
        got, m2 = uo.epoch(og, y, 7, seed=1, order=rng.permutation(int(m.sum())), **KW)
        assert got.tobytes() == ref.tobytes() and np.array_equal(m, m2)


def test_a_row_does_not_depend_on_the_order_of_the_other_rows(mix):
    """The rows 10 .. n - 1 stored in the reverse order (another matrix, whose rows 0 .. 9 are the same entries with
    the same numbers): the rows 0 .. 9 move the same way."""
    g, og = mix
    y = uo.random_init(og.n, 2, 2)
    ref, _ = uo.epoch(og, y, 3, **KW)
    rows = np.r_[np.arange(10), np.arange(og.n - 1, 9, -1)]
    h = sp.csr_matrix(g)[rows]
    oh = uo.Graph(sp.csr_matrix((h.data, h.indices, h.indptr), shape=g.shape))
    assert np.array_equal(oh.indptr[:11], og.indptr[:11])
    got, _ = uo.epoch(oh, y, 3, **KW)
    assert got[:10].tobytes() == ref[:10].tobytes()


def test_schedule_is_stateless_and_matches_the_counts(mix):
    _, og = mix
    fires = og.fires(50)
    assert 0 < fires.sum() < len(og.w)  # the short schedule drops the light entries
    count = np.zeros(len(og.w), dtype=np.int64)
    for t in range(50):
        count[og.active(t, 50)] += 1
    expect = np.where(fires, np.floor(49 / (og.w_max / np.where(og.w > 0, og.w, 1.0))), 0)
    assert np.array_equal(count, expect.astype(np.int64))
    # the mirror entry has the same schedule
    m = sp.csr_matrix((count, og.indices, og.indptr), shape=(og.n, og.n))
    assert (m != m.T).nnz == 0


def test_random_init_is_the_packages(mix):
    from infercnvpy_amd.tl._umap import random_init

    y = uo.random_init(1000, 3, 5)
    assert y.dtype == np.float32 and y.min() >= -10 and y.max() < 10 and abs(float(y.mean())) < 0.5
    assert random_init(1000, 3, 5).tobytes() == y.tobytes()
    assert random_init(1000, 3, 6).tobytes() != y.tobytes()


def test_spectral_init(mix):
    from infercnvpy_amd.tl._umap import spectral_init

    g, _ = mix
    y = spectral_init(g, 2, 0)
    assert y.shape == (300, 2) and y.dtype == np.float32 and abs(np.abs(y).max() - 10) < 1e-3
    assert spectral_init(g, 2, 0).tobytes() == y.tobytes()
    top = y[np.abs(y).argmax(axis=0), np.arange(2)]
    assert (top > 0).all()
    assert spectral_init(lo.cliques([5, 4]), 2, 0) is None  # two connected components


def test_neighbour_preservation():
    rng = np.random.default_rng(0)
    y = rng.normal(size=(200, 2))
    d = ((y[:, None] - y[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    knn = np.argsort(d, axis=1)[:, :14]
    assert uo.neighbour_preservation(knn, y, 14) == 1.0
    assert uo.neighbour_preservation(knn, y, 14, rows=np.arange(0, 200, 7), block=8) == 1.0
    assert uo.neighbour_preservation(knn, rng.normal(size=(200, 2)), 14) < 0.2


# ---- tl.umap / pl.umap: what fails before the GPU is touched ----------------------------------------------------------
def _adata(n=300, **kw):
    from infercnvpy_amd._compat import SimpleAnnData

    return SimpleAnnData(np.zeros((n, 3), dtype=np.float32), **kw)


def test_tl_umap_argument_errors(mix):
    import infercnvpy_amd as cnv

    g, _ = mix
    with pytest.raises(KeyError, match="Did you run `pp.neighbors`"):
        cnv.tl.umap(_adata())
    with pytest.raises(KeyError, match="Did you run `pp.neighbors`"):
        cnv.tl.umap(_adata(), obsp="nope")
    with pytest.raises(KeyError, match="Did you run `pp.neighbors`"):
        cnv.tl.umap(_adata(uns={"cnv_neighbors": {"connectivities_key": "gone"}}))
    for c in (1, 4, 2.5, "2", True):
        with pytest.raises(ValueError, match="n_components"):
            cnv.tl.umap(None, adjacency=g, n_components=c)
    with pytest.raises(ValueError, match="unsupported keyword.*method"):
        cnv.tl.umap(None, adjacency=g, method="rapids")
    with pytest.raises(ValueError, match="301 vertices"):
        cnv.tl.umap(_adata(), adjacency=sp.block_diag([g, sp.csr_matrix((1, 1))]).tocsr())
    with pytest.raises(ValueError, match="square"):
        cnv.tl.umap(None, adjacency=g[:10])
    with pytest.raises(ValueError, match="init_pos has shape"):
        cnv.tl.umap(None, adjacency=g, init_pos=np.zeros((300, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="init_pos has shape"):
        cnv.tl.umap(_adata(obsm={"start": np.zeros((300, 2))}), adjacency=g, init_pos="start", n_components=3)
    with pytest.raises(KeyError, match="init_pos"):
        cnv.tl.umap(_adata(), adjacency=g, init_pos="pca")
    with pytest.raises(ValueError, match="non-finite"):
        cnv.tl.umap(None, adjacency=g, init_pos=np.full((300, 2), np.nan))
    for kw in (dict(maxiter=0), dict(maxiter=2.5), dict(random_state=0.5), dict(negative_sample_rate=-1),
               dict(negative_sample_rate=65), dict(alpha=-1.0), dict(gamma=float("nan")), dict(a=1.0), dict(a=0.0, b=1.0),
               dict(spread=0.0), dict(min_dist=-1.0)):
        with pytest.raises(ValueError, match="tl.umap"):
            cnv.tl.umap(None, adjacency=g, **kw)
    with pytest.raises(ValueError, match="scipy sparse matrix or"):
        cnv.tl.umap(None, adjacency=g.toarray())


def test_pl_umap_errors_and_axes():
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import pandas as pd

    import infercnvpy_amd as cnv

    ad = _adata(50)
    with pytest.raises(KeyError, match="Did you run `tl.umap`"):
        cnv.pl.umap(ad)
    ad.obsm["X_cnv_umap"] = uo.random_init(50, 2, 0)
    with pytest.raises(KeyError, match="nope"):
        cnv.pl.umap(ad, color="nope")
    ad.obs["cnv_leiden"] = pd.Categorical.from_codes(np.arange(50) % 3, categories=["0", "1", "2"])
    ad.obs["cnv_score"] = np.linspace(0, 1, 50)
    try:
        ax = cnv.pl.umap(ad, color="cnv_leiden", s=3)
        assert len(ax.collections[0].get_offsets()) == 50
        assert [t.get_text() for t in ax.get_legend().get_texts()] == ["0", "1", "2"]
        n_axes = len(ax.figure.axes)
        ax2 = cnv.pl.umap(ad, color="cnv_score")
        assert len(ax2.figure.axes) == n_axes + 1 and ax2.get_legend() is None  # the colour bar
        _, own = plt.subplots()
        assert cnv.pl.umap(ad, ax=own, show=False) is own and len(own.collections[0].get_offsets()) == 50
    finally:
        plt.close("all")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_umap_workspace", "icv_umap_epochs"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)


def test_workspace_bytes_are_linear_and_validated():
    from infercnvpy_amd import _lib

    lib = _lib.load()

    def need(n, nnz, c):
        out = ctypes.c_int64(-1)
        rc = lib.icv_umap_workspace(n, nnz, c, ctypes.byref(out))
        return rc, out.value

    def up(x):
        return (x + 255) // 256 * 256

    for n, nnz, c in ((1, 0, 2), (7, 12, 3), (2000, 60000, 2), (200_000, 5_000_000, 3), (1 << 30, (1 << 31) - 1, 3)):
        assert need(n, nnz, c) == (_lib.ICV_OK, up(4 * n * c) + up(4 * (n + 1)) + 256)
        assert need(n, 0, c) == need(n, nnz, c)  # linear in n (each part rounded up to 256); nnz adds nothing
    for bad in ((0, 0, 2), (-1, 0, 2), ((1 << 30) + 1, 0, 2), (5, -1, 2), (5, 1 << 31, 2), (5, 0, 1), (5, 0, 4)):
        assert need(*bad)[0] == _lib.ICV_ERR_INVALID
        assert b"umap_workspace" in lib.icv_last_error()
    assert lib.icv_umap_workspace(5, 0, 2, None) == _lib.ICV_ERR_INVALID

"""GPU tests (``-m gpu``): tl.pca's two kernels at their tile and lane limits, against exact references
(tests/_pca_oracle.py; that the references are what they claim is asserted on the CPU in tests/test_pca_oracle.py).

icv_project (k_csr_project / k_dense_project) against ``project_oracle``, bit for bit: a float64 fma chain over the
row's stored entries in stored order, one subtraction of the shift, one cast -- more than one trip of the lane loop
(k > 64), 1 to 5 rows on workgroups of 4, all eight instantiations and every input kind, a row of 1 802 entries, several
slabs of host dense input, and through tl.pca with the eigenvectors it returns.

icv_gram_f64 against ``int_gram``, exactly: on small-integer input every partial sum is an integer below 2^53, so every
summation order (and the MFMA's own) gives the one exact answer, and a term dropped or added twice shows -- W and n at
and around the 64-column tile and the 32-cell LDS stage, a second trip of the launch-pair loop (more partial tiles than
256 MB holds: W = 5 761 with two blocks, W = 5 760 with three), and a Gram continued by a second call."""
import functools
import time

import numpy as np
import pytest
import scipy.sparse as sp

import _pca_oracle as po

pytestmark = pytest.mark.gpu

BLOCK = 8192  # ICV_GRAM_BLOCK


def _same(got, ref, what):
    """Equal dtype, shape and values (np.array_equal); the count of differing elements is printed first."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    bad = np.argwhere(got != ref)
    print(f"{what}: shape {got.shape}, {len(bad)} differ")
    assert np.array_equal(got, ref), (what, len(bad), bad[:4].tolist(), [(got[tuple(i)], ref[tuple(i)]) for i in bad[:4]])


# ---- icv_project ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lane_case():
    """9 x 70 at density 0.5 (row 0 full, row 1 empty), 130 components: the chain once, for every k and n below."""
    x, v, shift = po.projection_case(9, 70, 130, seed=1)
    chain = po.project_chain(x, v)
    n_diff = int(np.count_nonzero(po.muladd_chain(x, v) != chain))
    print(f"{n_diff} of {chain.size} results differ from the multiply-add chain")
    assert n_diff >= chain.size // 4  # a kernel that did not contract to fma would fail below
    return x, v, shift, chain


def _check_project(x, v, shift, chain, what):
    """Both output dtypes, with and without the shift, for the dense and the CSR form of ``x``."""
    from infercnvpy_amd import _engine

    for inp, kind in ((x, "dense"), (sp.csr_matrix(x), "csr")):
        for sh in (None, shift):
            for dt in (np.float64, np.float32):
                ref = po.project_oracle(x, v, sh, dt, chain=chain)
                _same(_engine.project(inp, v, sh, dt), ref, (what, kind, "shift" if sh is not None else "no shift", dt.__name__))


@pytest.mark.parametrize("k", [1, 63, 64, 65, 130])
def test_project_lane_trips(k):
    x, v, shift, chain = _lane_case()
    _check_project(x, np.ascontiguousarray(v[:, :k]), shift[:k], chain[:, :k], f"k={k}")


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_project_rows_per_workgroup(n):
    x, v, shift, chain = _lane_case()
    _check_project(x[:n], np.ascontiguousarray(v[:, :65]), shift[:65], chain[:n, :65], f"n={n}")


def test_project_every_instantiation_and_input_kind():
    import torch

    from infercnvpy_amd import _engine
    from infercnvpy_amd._engine import PackedCsr

    x, v, shift = po.projection_case(6, 70, 65, seed=2)
    x = x.astype(np.float32).astype(np.float64)  # float32 numbers: every input kind holds the same values
    c = sp.csr_matrix(x)
    data = c.data.copy()
    data[[3, 40, c.nnz - 1]] = 0.0  # stored zeros: no-ops
    data[7] = -0.0
    c = sp.csr_matrix((data, c.indices, c.indptr), shape=c.shape)
    assert c.nnz == np.count_nonzero(x) and c.has_canonical_format
    d = c.toarray()
    d[2, np.flatnonzero(d[2] == 0)[0]] = -0.0  # a dense -0.0 is skipped like +0.0
    assert np.signbit(d).sum() > np.count_nonzero(d < 0)
    chain = po.project_chain(c, v)
    _same(po.project_chain(d, v), chain, "oracle: dense against csr")

    def packed():
        return PackedCsr(torch.from_numpy(c.indptr.astype(np.int64)).cuda(), torch.from_numpy(c.indices.astype(np.int32)).cuda(),
                         torch.from_numpy(c.data.astype(np.float64)).cuda(), c.shape[1])

    kinds = {
        "host csr float32": lambda: c.astype(np.float32), "host csr float64": lambda: c,
        "host dense float32": lambda: d.astype(np.float32), "host dense float64": lambda: d,
        "cuda float32": lambda: torch.from_numpy(d.astype(np.float32)).cuda(), "cuda float64": lambda: torch.from_numpy(d).cuda(),
        "PackedCsr": packed,
    }
    assert c.astype(np.float32).nnz == c.nnz and np.signbit(d.astype(np.float32)).sum() == np.signbit(d).sum()
    for kind, make in kinds.items():
        for sh in (None, shift):
            for dt in (np.float64, np.float32):
                ref = po.project_oracle(c, v, sh, dt, chain=chain)
                _same(_engine.project(make(), v, sh, dt), ref, (kind, "shift" if sh is not None else "no shift", dt.__name__))


def test_project_realistic_row():
    """W = 1 802: one fully stored row and one at X_cnv's 13 %, 50 components."""
    x, v, shift = po.projection_case(2, 1802, 50, seed=3, density=0.13, full_row=0, empty_row=None)
    assert np.count_nonzero(x[0]) == 1802 and 150 < np.count_nonzero(x[1]) < 330
    _check_project(x, v, shift, po.project_chain(x, v), "W=1802")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_project_several_slabs(dtype, monkeypatch):
    """Host dense input in slabs of 3 rows (10 rows: the last slab holds one): ``out[r0:]`` with r0 = 3, 6, 9."""
    from infercnvpy_amd import _engine

    x, v, shift = po.projection_case(10, 70, 7, seed=4)
    x = x.astype(dtype)
    chain = po.project_chain(x, v)
    one = {(s is not None, dt): _engine.project(x, v, s, dt) for s in (None, shift) for dt in (np.float64, np.float32)}
    seen = []
    slabs = _engine._PcaInput.slabs
    monkeypatch.setattr(_engine._PcaInput, "slabs", lambda self, rows: (seen.append(rows), slabs(self, rows))[1])
    monkeypatch.setattr(_engine, "free_hbm_bytes", lambda: 3 * 4 * 70 * x.itemsize)
    for (has_shift, dt), ref in one.items():
        got = _engine.project(x, v, shift if has_shift else None, dt)
        _same(got, ref, ("slabs of 3 against one slab", dtype.__name__, has_shift, dt.__name__))
        _same(got, po.project_oracle(x, v, shift if has_shift else None, dt, chain=chain), ("slabs of 3 against the oracle",))
    assert seen == [3] * 4, seen


def _ad(x):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 1), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    return ad


def test_project_through_tl_pca():
    """130 components (three trips of the lane loop) through the public call; the eigen-solver is taken out of the
    comparison by projecting the oracle on the components the call returns."""
    import infercnvpy_amd as cnv

    x, _, _ = po.projection_case(300, 200, 1, seed=5, density=0.02, full_row=None, empty_row=7)
    xs = sp.csr_matrix(x)
    assert 900 < xs.nnz < 1500
    xp, comp, _, _ = cnv.tl.pca(_ad(xs), zero_center=False, n_comps=130, dtype="float64", inplace=False, return_info=True)
    assert comp.shape == (130, 200) and comp.dtype == np.float64
    chain = po.project_chain(xs, comp.T)
    _same(xp, po.project_oracle(xs, comp.T, chain=chain), "tl.pca float64")
    x32 = cnv.tl.pca(_ad(xs), zero_center=False, n_comps=130, inplace=False)
    _same(x32, po.project_oracle(xs, comp.T, dtype=np.float32, chain=chain), "tl.pca float32")
    _same(cnv.tl.pca(_ad(x), zero_center=False, n_comps=130, inplace=False), x32, "tl.pca float32, dense input")

    # centred: the shift comes from the device column sums, so the whole call against the SVD oracle
    got = cnv.tl.pca(_ad(xs), zero_center=True, n_comps=130, inplace=False)
    exp, _, _, _ = po.pca_oracle(x, 130, True)
    tol = po.ulp_tol(exp)
    print("zero_center=True: max |error| / tol", float(np.max(np.abs(got.astype(np.float64) - exp) / tol)))
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - exp) <= tol)


# ---- icv_gram_f64 -----------------------------------------------------------------------------------------------------
def _check_gram(inp, ref, what, zero_center=False, colsum=None):
    from infercnvpy_amd import _engine

    g, s = _engine.gram(inp, zero_center=zero_center)
    bad = int(np.count_nonzero(g != ref))
    print(f"{what}: G {g.shape}, {bad} differ from the integer Gram")
    assert g.dtype == np.float64 and g.shape == ref.shape
    assert np.array_equal(g, ref), (what, bad, np.argwhere(g != ref)[:4].tolist())
    assert np.array_equal(g, g.T), (what, "G is not symmetric")
    if zero_center:
        assert s.dtype == np.float64 and np.array_equal(s, colsum), (what, "column sums")
    return g


@pytest.mark.parametrize("w", [63, 64, 65, 127, 128, 129, 191, 192, 193])
def test_gram_tile_and_stage_edges(w):
    for n in (1, 31, 32, 33, 63, 64, 65):
        x = po.integer_matrix(n, w, seed=1000 * w + n, density=0.4)
        ref = po.int_gram(x)
        colsum = np.asarray(x.astype(np.int64).sum(axis=0)).ravel()
        assert x.dtype == np.float32 and np.count_nonzero(ref) > 0
        _check_gram(x, ref, (n, w, "csr float32"), True, colsum)  # float32 panel
        _check_gram(x.toarray().astype(np.float64), ref, (n, w, "dense float64"), True, colsum)  # float64 panel


def _two_block_matrix(n, w, density, seed):
    """Integer CSR (float32) whose last 33 rows and three rows of the first block are written densely into the same
    dozen columns, the last column among them: those Gram elements get terms from the first and from the last block."""
    x = po.integer_matrix(n, w, seed=seed, density=density).tolil()
    rng = np.random.RandomState(seed + 1)
    rows = np.r_[[5, 4000, BLOCK - 1], np.arange(n - 33, n)]
    cols = np.r_[[0, 1, 63, 64, 65, 127, 128], [w // 2, w - 66, w - 65, w - 2, w - 1]]
    x[np.ix_(rows, cols)] = (rng.randint(1, 8, size=(len(rows), len(cols))) * rng.choice([-1, 1], size=(len(rows), len(cols)))
                             ).astype(np.float32)
    x = x.tocsr()
    assert x.dtype == np.float32 and x.has_canonical_format
    return x


# n_t = 91 tiles a side: 4 186 partial tiles of 32 KiB are 130.8 MiB, one block per launch pair; n_t = 90: 127.97 MiB, two
@pytest.mark.parametrize("w, n, trips", [(5761, BLOCK + 33, 2), (5760, 2 * BLOCK + 33, 2)])
def test_gram_late_launch_pairs(w, n, trips, monkeypatch):
    from infercnvpy_amd import _engine

    t0 = time.perf_counter()
    n_t = -(-w // 64)
    per = max(1, (256 << 20) // (n_t * (n_t + 1) // 2 * 64 * 64 * 8))
    n_blocks = -(-n // BLOCK)
    assert -(-n_blocks // per) == trips and per < n_blocks  # the loop over launch pairs takes a second trip
    x = _two_block_matrix(n, w, 0.003, seed=w)
    last = (n_blocks - 1) * BLOCK
    both = po.int_gram(x[:BLOCK], dense=False).multiply(po.int_gram(x[last:], dense=False))
    assert both.nnz >= 100 and both[w - 1, 0] != 0  # elements with terms from the first and from the last block
    ref = po.int_gram(x)
    t1 = time.perf_counter()
    g = _check_gram(x, ref, (n, w, "one call"))
    del ref
    t2 = time.perf_counter()
    monkeypatch.setattr(_engine, "_gram_rows", lambda *a: BLOCK)  # one block per call: never a second trip
    g1, _ = _engine.gram(x)
    assert np.array_equal(g, g1), "one call and one block per call differ"
    print(f"{x.nnz} entries; reference {t1 - t0:.2f} s, one call {t2 - t1:.2f} s, block by block {time.perf_counter() - t2:.2f} s")


def test_gram_continued_by_a_second_call(monkeypatch):
    """8 192 + 40 rows at W = 129 split at row 8 192: the first call fills G, the second accumulates into it."""
    from infercnvpy_amd import _engine

    n, w = BLOCK + 40, 129
    x = po.integer_matrix(n, w, seed=6, density=0.4)
    d = x.toarray().astype(np.float64)
    ref = po.int_gram(x)
    assert np.count_nonzero(po.int_gram(x[:BLOCK]) * po.int_gram(x[BLOCK:])) > w * w // 2
    one = [_check_gram(inp, ref, (n, w, kind, "one call")) for inp, kind in ((x, "csr float32"), (d, "dense float64"))]
    calls = []
    lib_check = _engine._lib.check
    monkeypatch.setattr(_engine, "_gram_rows", lambda *a: BLOCK)
    monkeypatch.setattr(_engine._lib, "check", lambda rc: (calls.append(rc), lib_check(rc))[1])
    for (inp, kind), g in zip(((x, "csr float32"), (d, "dense float64")), one):
        del calls[:]
        g2 = _check_gram(inp, ref, (n, w, kind, "two calls"))
        assert len(calls) == 2, calls  # icv_gram_f64 ran twice (no column sums asked for)
        assert np.array_equal(g2, g)

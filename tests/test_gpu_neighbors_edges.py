"""GPU tests (``-m gpu``): pp.neighbors at the limits of its float32 sweep and of the fuzzy graph, against the numpy
oracle of DESIGN.md 4.9 (tests/_neighbors_oracle.py).  The inputs are the builders of the oracle file; the property that
makes each of them an edge is asserted on the CPU in tests/test_neighbors_oracle.py.  Equality is ``np.array_equal``.

What test_gpu_neighbors.py does not enter: one and two column parts of the candidate sweep, the magnitude gate (every
row through k_knn_exact), underflow and subnormal inputs, a row stride, a floored sigma on rows with rho > 0, a hub
row, connectivities that are float32 subnormals or round to 0, and the smoothing / symmetrisation kernels on their own
(the latter contain no exp and are compared for equality on hand-made weights)."""
import functools

import numpy as np
import pytest

import _neighbors_oracle as O

pytestmark = pytest.mark.gpu


def _adata(x, key="X_cnv_pca"):
    from infercnvpy_amd._compat import SimpleAnnData

    return SimpleAnnData(np.zeros((x.shape[0], 1), dtype=np.float32), obsm={key: x})


def _run(x, k):
    import infercnvpy_amd as cnv

    return cnv.pp.neighbors(_adata(x), n_neighbors=k, inplace=False, return_info=True)


def _check(x, k, got=None, what=""):
    """test_gpu_neighbors._check with ONE difference: a connectivity may differ from the oracle's by one float32 ulp,
    which is 2^-149 for a subnormal (there 2^-23 |ref| is less than the spacing of the numbers).  Returns the oracle's
    result."""
    n = x.shape[0]
    dist, conn, idx, kd, rho, sigma = got if got is not None else _run(x, k)
    exp = O.neighbors(x, k)
    assert idx.dtype == np.int32 and idx.shape == (n, k - 1) and kd.dtype == np.float32 and kd.shape == (n, k - 1)
    assert rho.dtype == np.float64 and rho.shape == (n,) and sigma.dtype == np.float64 and sigma.shape == (n,)
    bad = np.flatnonzero((idx != exp["knn_indices"]).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5]}: {idx[bad[:1]]} vs {exp['knn_indices'][bad[:1]]}"
    assert np.array_equal(kd, exp["knn_distances"]), what
    assert np.array_equal(rho, exp["rho"]), what
    pos = exp["rho"] > 0
    assert np.array_equal(sigma[pos], exp["sigma"][pos]), what
    tol = n * k * 2.0**-53
    assert np.all(np.abs(sigma[~pos] - exp["sigma"][~pos]) <= tol * exp["sigma"][~pos]), what
    for m in (dist, conn):
        assert m.format == "csr" and m.shape == (n, n) and m.dtype == np.float32
    e = exp["distances"]
    assert np.array_equal(dist.indptr, e.indptr) and np.array_equal(dist.indices, e.indices), what
    assert np.array_equal(dist.data, e.data), what
    e = exp["connectivities"]
    assert np.array_equal(conn.indptr, e.indptr) and np.array_equal(conn.indices, e.indices), what
    ref = e.data.astype(np.float64)
    assert np.all(np.abs(conn.data.astype(np.float64) - ref) <= np.maximum(2.0**-23 * np.abs(ref), 2.0**-149)), what
    assert conn.has_canonical_format and np.all(conn.data != 0)
    t = conn.T.tocsr()
    t.sort_indices()
    assert np.array_equal(t.indptr, conn.indptr) and np.array_equal(t.indices, conn.indices)
    assert np.array_equal(t.data, conn.data), f"{what}: connectivities not bitwise symmetric"
    return exp


def _knn(x, k, stage_ms=None):
    """_engine.knn of the host array: (indices, distances, n_exact) on the host."""
    import torch

    from infercnvpy_amd import _engine

    idx, dist, n_exact = _engine.knn(torch.from_numpy(x).cuda(), k, stage_ms=stage_ms)
    return idx.cpu().numpy(), dist.cpu().numpy(), n_exact


@functools.lru_cache(maxsize=None)
def _unscaled_indices(n, d, k, seed):
    """knn_indices of the GPU run on mixture(n, d, seed) at unit scale (computed once per shape)."""
    idx = _run(O.mixture(n, d, seed=seed), k)[2]
    idx.setflags(write=False)
    return idx


# ---- 1. one and two column parts ---------------------------------------------------------------------------------------
def _geom(n, d, k):
    """KnnGeom of csrc/icv_api.hip restated: (parts, chunk, workspace bytes).  The bytes tie this copy to the library:
    icv_knn_workspace has to return the same number."""
    rows, max_parts, slack = 128, 16, 8
    n_pad = (n + rows - 1) // rows * rows
    want = min(max(2048 // (n_pad // rows), 1), max_parts)
    chunk = ((n_pad + want - 1) // want + 31) // 32 * 32
    parts = (n_pad + chunk - 1) // chunk
    dp = 64 if d <= 64 else 128 if d <= 128 else 256
    L = k - 1 + slack
    rows_per = max((n + 1023) // 1024, 64)
    n_slabs = (n + rows_per - 1) // rows_per
    segs = (n_slabs * d * 8, 256 * 4, 16, n_pad * dp * 4, n_pad * 4, n * parts * 2 * L * 4, n * parts * 2 * 4, n * 4)
    return parts, chunk, sum((b + 255) // 256 * 256 for b in segs)


@pytest.mark.parametrize("n,seed,parts", [(131_200, 3, 1), (100_000, 4, 2)])
def test_one_and_two_column_parts(n, seed, parts):
    import ctypes

    import torch

    from infercnvpy_amd import _engine, _lib

    d, k = 8, 15
    g_parts, chunk, g_bytes = _geom(n, d, k)
    need = ctypes.c_int64(-1)
    assert _lib.load().icv_knn_workspace(n, d, k, ctypes.byref(need)) == _lib.ICV_OK
    assert g_parts == parts, f"KnnGeom's part count changed: {g_parts} part(s) at n={n}, this case was chosen for {parts}"
    assert need.value == g_bytes, (f"icv_knn_workspace asks for {need.value} bytes, the restated KnnGeom for {g_bytes}: "
                                   "the library's part count, chunk or workspace layout is no longer the one restated here")
    x = O.mixture(n, d, seed=seed)
    ms = []
    idx_d, dist_d, n_exact = _engine.knn(torch.from_numpy(x).cuda(), k, stage_ms=ms)
    print(f"n={n}: {parts} part(s) of {chunk} columns, rows sent to the exact kernel: {n_exact}, "
          f"centring / sweep / re-rank / exact ms: {[round(v, 3) for v in ms]}")

    # every row, on the device
    assert idx_d.shape == (n, k - 1) and dist_d.shape == (n, k - 1)
    assert bool(((idx_d >= 0) & (idx_d < n)).all())
    assert not bool((idx_d == torch.arange(n, device="cuda", dtype=torch.int32)[:, None]).any()), "a row lists itself"
    assert bool((torch.diff(torch.sort(idx_d, dim=1).values, dim=1) > 0).all()), "a row lists a cell twice"
    assert bool((torch.diff(dist_d, dim=1) >= 0).all()), "distances not ascending"
    assert n_exact < 0.01 * n

    # 256 sampled rows against the oracle, then the columns at both ends of every part (whole 32-column tiles) and the
    # rows that must list them: their nearest neighbours
    idx, dist = idx_d.cpu().numpy(), dist_d.cpu().numpy()
    rows = np.sort(np.random.default_rng(seed).choice(n, 256, replace=False))
    ends = np.concatenate([np.arange(p * chunk, p * chunk + 32) for p in range(parts)]
                          + [np.arange(min(n, (p + 1) * chunk) - 32, min(n, (p + 1) * chunk)) for p in range(parts)])
    blocks = [rows[:128], rows[128:]] + [ends[b:b + 128] for b in range(0, len(ends), 128)]
    listing = []
    for b, rr in enumerate(blocks):
        e_idx, e_d2 = O._knn_block(x, rr, k - 1)
        assert np.array_equal(idx[rr], e_idx), f"block {b}: rows {rr[(idx[rr] != e_idx).any(axis=1)][:5]}"
        assert np.array_equal(dist[rr], np.sqrt(e_d2).astype(np.float32)), f"block {b}"
        if b >= 2:
            listing.append(e_idx[:, 0])
    rr = np.unique(np.concatenate(listing))[:128]
    e_idx, e_d2 = O._knn_block(x, rr, k - 1)
    assert np.array_equal(idx[rr], e_idx), f"rows next to the part ends: {rr[(idx[rr] != e_idx).any(axis=1)][:5]}"
    assert np.array_equal(dist[rr], np.sqrt(e_d2).astype(np.float32))


# ---- 2. / 3. the magnitude gate, overflow, underflow ---------------------------------------------------------------------
EXACT_CASES = [(2, 1, 2, 60), (17, 3, 15, 60), (65, 65, 64, 60), (257, 256, 30, 60), (1000, 50, 15, 60), (3000, 2, 64, 60),
               (1000, 50, 15, 100)]


@pytest.mark.parametrize("n,d,k,p", EXACT_CASES)
def test_exact_kernel_produces_the_whole_result(n, d, k, p):
    seed = 1 if (n, d) == (1000, 50) else 0
    x = O.mixture(n, d, seed=seed)
    xs = O.scaled(x, p)
    x64 = xs.astype(np.float64)
    assert np.isfinite(xs).all() and ((x64 - x64.mean(axis=0)) ** 2).sum(axis=1).max() >= 4e36  # past the 1e36 gate
    idx, dist, n_exact = _knn(xs, k)
    print(f"n={n} d={d} k={k} p={p}: rows sent to the exact kernel: {n_exact}")
    assert n_exact == n
    # before anything walks these indices: k_knn_exact wrote a cell of [0, n) everywhere, and the right one
    assert idx.min() >= 0 and idx.max() < n
    e_idx, e_dist, _ = O.knn(xs, k)
    assert np.array_equal(idx, e_idx) and np.array_equal(dist, e_dist)
    got = _run(xs, k)
    assert np.array_equal(got[2], idx) and np.array_equal(got[3], dist)
    _check(xs, k, got=got, what=f"n={n} d={d} k={k} p={p}")
    assert np.array_equal(idx, _unscaled_indices(n, d, k, seed))


@pytest.mark.parametrize("p", [-70, -100, -120])
def test_underflow(p):
    n, d, k = 1000, 50, 15
    xs = O.scaled(O.mixture(n, d, seed=1), p)
    idx, dist, n_exact = _knn(xs, k)
    print(f"p={p}: rows sent to the exact kernel: {n_exact} of {n}")
    assert idx.min() >= 0 and idx.max() < n
    got = _run(xs, k)
    _check(xs, k, got=got, what=f"p={p}")
    assert np.array_equal(got[2], idx) and np.array_equal(got[3], dist)
    assert np.array_equal(idx, _unscaled_indices(n, d, k, 1))


# ---- 4. distances far below the float32 keys; nothing but ties ------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 15, 64])
def test_near_duplicates(k):
    _check(O.near_duplicates(), k, what=f"near duplicates k={k}")


@pytest.mark.parametrize("k", [2, 15, 64])
def test_simplex(k):
    x = O.simplex(64)
    got = _run(x, k)
    exp = _check(x, k, got=got, what=f"simplex k={k}")
    assert np.all(exp["rho"] > 0) and np.array_equal(got[5], exp["sigma"])
    if k == 2:
        # one neighbour: s = exp(0) = 1 = log2(2) at the first step, the bisection stops at mid = 1 and nothing is
        # floored; from two neighbours on s >= 2 ... > log2(k) never comes down and mid halves to 2^-64
        assert not exp["floored"].any() and np.all(got[5] == 1.0)
    else:
        assert exp["floored"].all()


# ---- 5. row stride --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [50, 1])
def test_row_stride(d):
    import torch

    from infercnvpy_amd import _engine

    n, k = 1000, 15
    for p in (0, 60):  # the sweep and the re-rank read with the stride; past the magnitude gate k_knn_exact does
        x = O.scaled(O.mixture(n, d, seed=20 + d), p)
        wide = np.full((n, d + 3), 3e38, dtype=np.float32)  # what must not be read
        wide[:, :d] = x
        wide = torch.from_numpy(wide).cuda()
        view = wide[:, :d]
        assert view.stride(0) == d + 3 and view.stride(1) == 1
        idx_c, dist_c, ne_c = _engine.knn(torch.from_numpy(x).cuda(), k)
        idx_s, dist_s, ne_s = _engine.knn(view, k)
        print(f"d={d} p={p}: rows sent to the exact kernel: {ne_c} contiguous, {ne_s} strided")
        assert ne_s == ne_c and (ne_c == n if p else ne_c < n)
        assert torch.equal(idx_s, idx_c) and torch.equal(dist_s.view(torch.int32), dist_c.view(torch.int32))
        e_idx, e_dist, _ = O.knn(x, k)
        assert np.array_equal(idx_s.cpu().numpy(), e_idx) and np.array_equal(dist_s.cpu().numpy(), e_dist)


# ---- 6. hub row, weights that are 0 or subnormal in float32 ------------------------------------------------------------
def test_hub_row():
    x = O.hub()
    got = _run(x, 15)
    _check(x, 15, got=got, what="hub")
    print(f"hub row length: {got[1].indptr[1]}")
    assert got[1].indptr[1] == x.shape[0] - 1


def test_small_clusters_drop_the_zero_weights():
    x = O.small_clusters()
    got = _run(x, 15)
    exp = _check(x, 15, got=got, what="small clusters")
    assert np.all(np.diff(got[1].indptr) == 9) and exp["floored"].all()


def test_ladder_stores_subnormals_and_drops_zeros():
    x = O.ladder()
    got = _run(x, O.LADDER_K)
    _check(x, O.LADDER_K, got=got, what="ladder")
    conn = got[1]
    n_sub = int((conn.data < np.finfo(np.float32).tiny).sum())
    n_drop = int((got[2][:12] >= 12).sum()) - conn[:12, 12:].nnz
    print(f"ladder: {n_sub} subnormal connectivities stored, {n_drop} cluster-to-rung entries dropped as 0")
    assert n_sub >= 5 and n_drop >= 5


# ---- 7. the symmetrisation kernels alone, for equality ----------------------------------------------------------------
EXTREMES = [0.0, 1.0, 2.0**-149, 2.0**-150, 2.0**-150 * (1 + 2.0**-52), 1.5 * 2.0**-149, 2.0**-126]


def _sym_indices(n, k, variant, rng):
    km1 = k - 1
    if variant == "cyclic":  # the next k - 1 cells: fully mutual for small n
        return ((np.arange(n)[:, None] + 1 + np.arange(km1)[None, :]) % n).astype(np.int32)
    idx = np.empty((n, km1), dtype=np.int32)
    for i in range(n):
        if variant == "random":
            r = rng.choice(n - 1, km1, replace=False)
            idx[i] = r + (r >= i)
        elif i == 0:  # "hub", "hub_full": every other row lists cell 0
            idx[i] = 1 + rng.choice(n - 1, km1, replace=False)
        else:
            r = 1 + rng.choice(n - 2, km1 - 1, replace=False)  # the cells but 0 and i
            idx[i] = rng.permutation(np.append(r + (r >= i), 0))
    return idx


@pytest.mark.parametrize("variant", ["random", "hub", "hub_full", "cyclic"])
@pytest.mark.parametrize("n", [2, 3, 64, 65, 1000, 5000])
def test_symmetrise_kernels_alone(n, variant):
    import torch

    from infercnvpy_amd import _engine

    for k in (2, 15, 64):
        if k > n:
            continue
        rng = np.random.default_rng(100 * n + k)
        idx = _sym_indices(n, k, variant, rng)
        assert not (idx == np.arange(n)[:, None]).any() and idx.min() >= 0 and idx.max() < n
        assert np.all(np.diff(np.sort(idx, axis=1), axis=1) > 0)
        if variant in ("hub", "hub_full"):
            assert (idx[1:] == 0).sum() == n - 1
        if variant == "hub_full":  # normal float32 numbers only: nothing is dropped and row 0 keeps all n - 1 entries
            w = 0.25 + 0.5 * rng.random(idx.shape)
        else:
            w = rng.random(idx.shape)
            pick = rng.random(idx.shape) < 0.5
            w[pick] = rng.choice(EXTREMES, size=int(pick.sum()))
        what = f"n={n} k={k} {variant}"
        e = O.connectivities_csr(idx, w)
        indptr, indices, data = (t.cpu().numpy() for t in
                                 _engine.knn_symmetrize(torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda(), k))
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
        assert np.array_equal(indptr, e.indptr), what
        assert np.array_equal(indices, e.indices), what
        assert np.array_equal(data, e.data), what
        assert np.all(data != 0)
        if variant == "hub" and n > 2:
            assert indptr[1] == np.count_nonzero(e[0].toarray()) >= (n - 1) // 2  # the long row
        if variant == "hub_full":
            assert indptr[1] == n - 1 and indptr[-1] == e.nnz  # the row of full length, every entry stored
        dist = rng.random(idx.shape).astype(np.float32)
        dist[rng.random(idx.shape) < 0.2] = 0.0  # distances keep their explicit zeros
        e = O.distances_csr(idx, dist)
        indptr, indices, data = (t.cpu().numpy() for t in
                                 _engine.knn_sorted_rows(torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda()))
        assert np.array_equal(indptr, e.indptr) and np.array_equal(indices, e.indices), what
        assert np.array_equal(data, e.data), what


# ---- 8. k_knn_smooth alone ----------------------------------------------------------------------------------------------
def _smooth_rows(n, km1, rng):
    """Ascending float32 distance rows, by row number modulo 5: all zeros, all equal, one zero and then equal values, a
    geometric spread over 30 decades, ordinary rows."""
    d = np.sort(np.abs(rng.normal(size=(n, km1))) + 0.1, axis=1)
    i = np.arange(n)
    d[i % 5 == 0] = 0.0
    d[i % 5 == 1] = rng.random(((i % 5 == 1).sum(), 1)) + 0.5
    d[i % 5 == 2] = rng.random(((i % 5 == 2).sum(), 1)) + 0.5
    d[i % 5 == 2, 0] = 0.0
    d[i % 5 == 3] = np.sort(10.0 ** rng.uniform(-15, 15, size=((i % 5 == 3).sum(), km1)), axis=1)
    return d.astype(np.float32)


def _bisection_margins(row, k):
    """The oracle's s - log2(k) at every step of the bisection of one row (for the message of a sigma mismatch)."""
    delta = row.astype(np.float64)
    rho = delta[delta > 0].min() if (delta > 0).any() else 0.0
    g = np.maximum(delta - rho, 0.0)
    lo, hi, mid, out = 0.0, np.inf, 1.0, []
    for _ in range(64):
        s = float(O._seq_sum(np.exp(-(g / mid))[None, :])[0]) - np.log2(float(k))
        out.append(s)
        if abs(s) < 1e-5:
            break
        if s > 0:
            hi = mid
            mid = (lo + hi) / 2.0
        else:
            lo = mid
            mid = mid * 2.0 if np.isinf(hi) else (lo + hi) / 2.0
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_smooth_kernel_alone(n):
    import torch

    from infercnvpy_amd import _engine

    for k in (2, 15, 64):
        rng = np.random.default_rng(1000 * n + k)
        dist = _smooth_rows(n, k - 1, rng)
        assert np.all(np.diff(dist, axis=1) >= 0)
        rho, sigma, w = (t.cpu().numpy() for t in _engine.knn_fuzzy(torch.from_numpy(dist).cuda(), k))
        e_rho, e_sigma, e_w, e_floored = O.smooth(dist, k)
        what = f"n={n} k={k}"
        print(f"{what}: floored rows {int(e_floored.sum())}, of them with rho > 0: {int((e_floored & (e_rho > 0)).sum())}")
        assert np.array_equal(rho, e_rho), what
        pos = e_rho > 0
        for i in np.flatnonzero(pos & (sigma != e_sigma))[:3]:
            m = np.array(_bisection_margins(dist[i], k))
            print(f"{what} row {i}: sigma {sigma[i]!r} vs {e_sigma[i]!r}; the oracle's s - target nearest to 0 / to "
                  f"+-1e-5: {np.abs(m).min():.3e} / {np.abs(np.abs(m) - 1e-5).min():.3e}")
        assert np.array_equal(sigma[pos], e_sigma[pos]), what
        tol = n * k * 2.0**-53
        assert np.all(np.abs(sigma[~pos] - e_sigma[~pos]) <= tol * e_sigma[~pos]), what
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(e_w == w, 0.0, np.abs(w - e_w) / np.abs(e_w))
        print(f"{what}: largest weight difference {rel.max() * 2.0**52:.3f} x 2^-52 relative")
        assert np.all(np.abs(w - e_w) <= 2.0**-52 * np.abs(e_w)), what
        if n >= 255 and k > 2:
            assert (e_floored & pos).any() and (~pos).any()  # a floored sigma on a row with rho > 0 is covered

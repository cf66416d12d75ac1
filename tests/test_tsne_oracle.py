"""The numpy oracle of tl.tsne against sklearn's own pieces (affinities, gradient, update rule, full
runs), and the new C-ABI symbols as far as they need no GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial.distance import squareform

import _neighbors_oracle as no
import _tsne_oracle as to
import _umap_oracle as uo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The largest relative difference of an entry of P between the oracle and sklearn 1.7.2's _joint_probabilities_nn on
# the six inputs below, measured: 1.2946e-3, at (2000 cells, perplexity 5) on an entry of 4e-31; the other five inputs
# stay below 3.8e-4.  sklearn stops its bisection at an entropy error of 1e-5; that row's error of 6.9e-6 predicts
# 1.31e-3 for this entry (d ln beta = dH / Var(beta rel) = 1.9e-5, times beta rel - mean = 68), so the difference is
# sklearn's tolerance, not the oracle's (whose rows meet the perplexity within 4e-15).
SKLEARN_P_MEASURED = 1.2946e-3
SKLEARN_P_BOUND = 4 * SKLEARN_P_MEASURED
# neighbour preservation (k = 14) of sklearn 1.7.2's TSNE(perplexity=30, early_exaggeration=12, learning_rate=1000,
# init="random") on no.mixture(500, 10, 0), seeds 0-4 (max |y| 38.0 .. 45.7):
SK500_BH = (0.57400, 0.57329, 0.58029, 0.56671, 0.56700)
SK500_EXACT = (0.56471, 0.56900, 0.57329, 0.57543, 0.56743)
SK500_MIN = min(SK500_BH + SK500_EXACT)
SK500_SPREAD = max(SK500_BH + SK500_EXACT) - SK500_MIN
_cache = {}


def _nb(n):
    if n not in _cache:
        x = no.mixture(n, 10, 0)
        _cache[n] = (x,) + no.knn(x, 64)[:2]
    return _cache[n]


def test_written_exponential():
    x = np.r_[np.linspace(-708, 5, 20001), -0.0, 0.0, -708.0000001, -1e300, -np.inf, np.nan]
    got = to.exp_(x)
    assert got[-1] == 0 and got[-2] == 0 and got[-3] == 0 and got[-4] == 0 and got[-5] == 1 and got[-6] == 1
    assert np.max(np.abs(got[:20001] / np.exp(x[:20001]) - 1)) < 4 * 2.0 ** -53


@pytest.mark.parametrize("n", (500, 2000))
def test_affinities_against_sklearn(n):
    from sklearn.manifold import _t_sne

    _, idx, dist = _nb(n)
    for perplexity in (5, 20, 30):
        beta, p = to.affinities(dist, perplexity)
        assert np.isfinite(beta).all() and (beta > 0).all() and (p >= 0).all()
        H = -(p * np.log2(np.where(p > 0, p, 1.0))).sum(axis=1)
        assert np.max(np.abs(2.0 ** H / perplexity - 1.0)) <= 1e-9
        w = to.symmetrize(idx, p)
        assert w.dtype == np.float32 and (w != w.T).nnz == 0 and w.has_canonical_format
        P = w.astype(np.float64) / (2.0 * n)
        assert abs(P.sum() - 1.0) <= w.nnz * 2.0 ** -24 / (2.0 * n) * float(w.max())
        d2 = no.distances_csr(idx, dist).astype(np.float64)
        d2.data = d2.data ** 2
        ref = sp.csr_matrix(_t_sne._joint_probabilities_nn(d2, perplexity, 0))
        ref.sort_indices()
        assert np.array_equal(ref.indices, P.indices) and np.array_equal(ref.indptr, P.indptr)
        rel = np.abs(P.data - ref.data) / ref.data
        print(f"n={n} perplexity={perplexity}: largest relative difference to sklearn {rel.max():.4e}")
        assert rel.max() <= SKLEARN_P_BOUND


def test_flat_rows_and_ties():
    d = np.ones((3, 7), dtype=np.float32)
    d[1] = 0.0
    d[2, 3:] = 2.0  # three neighbours tie at the front: the entropy never falls below log 3 > log 2
    beta, p = to.affinities(d, 2.0)
    assert np.array_equal(beta[:2], [1.0, 1.0]) and np.array_equal(p[:2], np.full((2, 7), 1.0 / 7))
    assert beta[2] == 2.0 ** 63 and np.array_equal(p[2], [1 / 3, 1 / 3, 1 / 3, 0, 0, 0, 0])


ROUNDINGS = {2: 15, 3: 17}
"""Rule 4's chain has 9 (c = 2) / 12 (c = 3) float32 roundings; weighted by how they reach q q dx_c (those inside d2
count twice, q = 1 / (1 + d2) enters squared): 2 (c + 2) for d2, 2 for 1 + d2, 2 for the division, 1 each for q q, the
product with dx_c and dx_c itself = 2 c + 11."""


@pytest.mark.parametrize("c", (2, 3))
@pytest.mark.parametrize("n", (200, 500))
def test_gradient_against_sklearn(n, c):
    from sklearn.manifold import _t_sne

    x = no.mixture(n, 10, 1)
    kk = to.n_neighbors(n, 30.0)
    idx, dist, _ = no.knn(x, kk + 1)
    w = to.symmetrize(idx, to.affinities(dist, 30.0)[1])
    og = to.Graph(w)
    P = squareform((w.astype(np.float64) / (2.0 * n)).toarray(), checks=False)
    rng = np.random.default_rng(n + c)
    for scale in (1e-4, 1.0, 50.0):
        y = (rng.normal(size=(n, c)) * scale).astype(np.float32)
        for ex in (1.0, 12.0):
            got = to.gradient(og, y, ex)
            _, ref = _t_sne._kl_divergence(y.astype(np.float64).ravel(), P * ex, 1.0, n, c)
            Zr, R, t_abs = to.repulsion(y, return_abs=True)
            Z = to.normaliser(Zr)
            A, a_abs = to.attraction(og, y, return_abs=True)
            m = np.diff(og.indptr)[:, None]
            eps_z = (c + 4) * 2.0 ** -24 + n * (n - 1) * 2.0 ** -33 / Z
            rep = np.abs(R.astype(np.float64)) * 2.0 ** -32 / Z
            tol = 4.0 * ((ex / (2.0 * n)) * (8 * 2.0 ** -53 * a_abs + m * 2.0 ** -41)
                         + (ROUNDINGS[c] * 2.0 ** -24 * t_abs + (n - 1) * 2.0 ** -33) / Z + rep * eps_z
                         + n * 2.0 ** -52 * ((ex / (2.0 * n)) * a_abs + t_abs / Z))  # sklearn's own float64 sums
            err = np.abs(got - ref.reshape(n, c))
            assert (err <= tol).all(), (scale, ex, float((err / tol).max()))
            assert np.abs(got).max() > 0 and (tol <= 1e-5 * np.abs(got).max()).all()  # the bound says something


def _sklearn_update(p, update, gains, grad, it, *, exploration=250, learning_rate=1000.0, min_gain=0.01):
    """sklearn.manifold._t_sne._gradient_descent's loop body, literally (momentum 0.5, then 0.8 as TSNE._tsne calls
    it), with the float32 storage of the contract."""
    momentum = 0.5 if it < exploration else 0.8
    p, update, gains = (a.astype(np.float64) for a in (p, update, gains))
    grad = grad.copy()
    inc = update * grad < 0.0
    dec = np.invert(inc)
    gains[inc] += 0.2
    gains[dec] *= 0.8
    np.clip(gains, min_gain, np.inf, out=gains)
    gains = gains.astype(np.float32)
    grad *= gains.astype(np.float64)
    update = (momentum * update - learning_rate * grad).astype(np.float32)
    p = (p + update.astype(np.float64)).astype(np.float32)
    return p, update, gains


def test_update_rule_is_sklearns():
    x = no.mixture(200, 10, 2)
    idx, dist, _ = no.knn(x, 64)
    og = to.Graph(to.symmetrize(idx, to.affinities(dist, 30.0)[1]))
    for c in (2, 3):
        state = to.run(og, to.start(to.random_init(200, c, 1)), 0, 5)
        mine = state
        for t in range(240, 260):
            ex = 12.0 if t < 250 else 1.0
            assert to.schedule(t) == (ex, 0.5 if t < 250 else 0.8)
            grad = to.gradient(og, state[0], ex)
            state = _sklearn_update(*state, grad, t)
            mine = to.iteration(og, *mine, t)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, state)), (c, t)
        assert (mine[2] != 1).any() and (mine[1] != 0).any()


def test_run_is_stateless_and_repulsion_is_order_free():
    x = no.mixture(120, 10, 3)
    idx, dist, _ = no.knn(x, 64)
    og = to.Graph(to.symmetrize(idx, to.affinities(dist, 20.0)[1]))
    s0 = to.start(to.random_init(120, 2, 0))
    whole = to.run(og, s0, 0, 8, exaggeration_iters=4)
    s = s0
    for t in range(8):
        s = to.run(og, s, t, t + 1, exaggeration_iters=4)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, s))
    Zr, R = to.repulsion(whole[0], block=512)
    Zr2, R2 = to.repulsion(whole[0], block=7)
    assert np.array_equal(Zr, Zr2) and np.array_equal(R, R2)
    perm = np.random.default_rng(0).permutation(120)
    Zr3, R3 = to.repulsion(whole[0][perm])
    assert np.array_equal(Zr3, Zr[perm]) and np.array_equal(R3, R[perm])
    same = np.zeros((9, 3), dtype=np.float32) + np.float32(0.37)
    Zr, R = to.repulsion(same)
    assert (Zr == 8 << 32).all() and not R.any()


def test_full_run_quality_against_sklearn():
    """The oracle's full runs must reach sklearn's minimum minus sklearn's own spread (SK500_*)."""
    x, _, _ = _nb(500)
    knn15 = no.knn(x, 15)[0]
    bound = SK500_MIN - SK500_SPREAD
    for kw in (dict(init_pos="random", random_state=0), dict(init_pos="pca")):
        y, _ = to.tsne(x, **kw)
        p = uo.neighbour_preservation(knn15, y, 14)
        print(f"{kw}: preservation {p:.5f} (bound {bound:.5f}), max |y| {np.abs(y).max():.2f}")
        assert np.isfinite(y).all() and np.abs(y).max() < 2 * 45.7 and p >= bound


def test_initial_positions_are_the_packages():
    from infercnvpy_amd.tl._tsne import pca_init, random_init

    y = to.random_init(1000, 3, 5)
    assert y.dtype == np.float32 and abs(float(y.std()) - 1e-4) < 5e-6 and abs(float(y.mean())) < 1e-5
    assert random_init(1000, 3, 5).tobytes() == y.tobytes() and random_init(1000, 3, 6).tobytes() != y.tobytes()
    assert uo.random_init(1000, 3, 5).tobytes() != (y * np.float32(1e5)).tobytes()  # another tag than tl.umap's
    x = no.mixture(300, 10, 0)
    p = pca_init(x, 2)
    assert p.tobytes() == to.pca_init(x, 2).tobytes() and abs(float(p[:, 0].std()) - 1e-4) < 1e-9
    with pytest.raises(ValueError, match="init_pos='pca'"):
        pca_init(x[:, :2], 3)
    with pytest.raises(ValueError, match="constant"):
        pca_init(np.ones((5, 3), dtype=np.float32), 2)


def test_tl_tsne_argument_errors():
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    x = no.mixture(100, 10, 0)
    ad = SimpleAnnData(np.zeros((100, 3), dtype=np.float32), obsm={"X_cnv_pca": x})
    for c in (1, 4, 2.5, "2", True):
        with pytest.raises(ValueError, match="n_components"):
            cnv.tl.tsne(ad, n_components=c)
    with pytest.raises(ValueError, match="unsupported keyword.*n_jobs"):
        cnv.tl.tsne(ad, n_jobs=4)
    with pytest.raises(ValueError, match="random_state"):
        cnv.tl.tsne(ad, random_state=0.5)
    with pytest.raises(ValueError, match="perplexity"):
        cnv.tl.tsne(ad, perplexity=63)
    with pytest.raises(ValueError, match="perplexity"):
        cnv.tl.tsne(ad, perplexity=0)
    with pytest.raises(ValueError, match="max_iter"):
        cnv.tl.tsne(ad, max_iter=2.5)
    with pytest.raises(ValueError, match="n_pcs"):
        cnv.tl.tsne(ad, n_pcs=11)
    with pytest.raises(KeyError, match="X_nope"):
        cnv.tl.tsne(ad, use_rep="nope")
    with pytest.raises(KeyError, match="init_pos"):
        cnv.tl.tsne(ad, init_pos="spectral")
    with pytest.raises(ValueError, match="init_pos has shape"):
        cnv.tl.tsne(ad, init_pos=np.zeros((100, 3)))
    with pytest.raises(ValueError, match="non-finite"):
        cnv.tl.tsne(ad, init_pos=np.full((100, 2), np.inf))
    with pytest.raises(ValueError, match="NaN or infinity"):
        cnv.tl.tsne(None, use_rep=np.full((100, 4), np.nan))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
NEW = ("icv_tsne_affinities", "icv_tsne_symmetrize_count", "icv_tsne_symmetrize_fill", "icv_tsne_workspace",
       "icv_tsne_iterations")


def test_symbols_are_exported_and_declared():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)


def test_workspace_bytes_are_linear_and_validated():
    from infercnvpy_amd import _lib

    lib = _lib.load()

    def need(n, nnz, c):
        out = ctypes.c_int64(-1)
        rc = lib.icv_tsne_workspace(n, nnz, c, ctypes.byref(out))
        return rc, out.value

    def up(x):
        return (x + 255) // 256 * 256

    for n, nnz, c in ((1, 0, 2), (7, 12, 3), (2000, 60000, 2), (200_000, 5_000_000, 3), (1 << 30, (1 << 31) - 1, 3)):
        expect = (3 * up(4 * n * c) + 2 * (up(8 * n) + up(8 * n * c) + 256) + up(4 * math.ceil(n / 256))
                  + up(4 * (n + 1)) + 256)
        assert need(n, nnz, c) == (_lib.ICV_OK, expect)
        assert need(n, 0, c) == need(n, nnz, c)  # nnz adds nothing
    for bad in ((0, 0, 2), (-1, 0, 2), ((1 << 30) + 1, 0, 2), (5, -1, 2), (5, 1 << 31, 2), (5, 0, 1), (5, 0, 4)):
        assert need(*bad)[0] == _lib.ICV_ERR_INVALID
        assert b"tsne_workspace" in lib.icv_last_error()
    assert lib.icv_tsne_workspace(5, 0, 2, None) == _lib.ICV_ERR_INVALID


def test_argument_checks_need_no_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(256)  # never dereferenced: the arguments are refused first
    assert lib.icv_tsne_affinities(None, 5, 3, 2.0, one, one, None) == _lib.ICV_ERR_INVALID
    for k, perplexity in ((0, 0.5), (64, 30.0), (10, 10.0), (10, 0.0), (10, float("nan"))):
        assert lib.icv_tsne_affinities(one, 5, k, perplexity, one, one, None) == _lib.ICV_ERR_INVALID
        assert b"tsne_affinities" in lib.icv_last_error()
    assert lib.icv_tsne_symmetrize_count(one, one, 0, 3, one, None) == _lib.ICV_ERR_INVALID
    assert lib.icv_tsne_symmetrize_fill(one, one, 5, 3, one, 31, one, one, None) == _lib.ICV_ERR_INVALID
    for kw in (dict(c=4), dict(ex=0.0), dict(eta=float("inf")), dict(t0=-1), dict(t0=3, t1=2), dict(n=0), dict(exi=-1)):
        a = dict(n=5, c=2, ex=12.0, exi=250, eta=1000.0, t0=0, t1=1)
        a.update(kw)
        rc = lib.icv_tsne_iterations(one, one, one, a["n"], 4, a["c"], a["ex"], a["exi"], a["eta"], a["t0"], a["t1"], one,
                                     one, one, one, None, None)
        assert rc == _lib.ICV_ERR_INVALID and b"tsne_iterations" in lib.icv_last_error()


# ---- the geometry of the device's grid and the inputs of tests/test_gpu_tsne_edges.py ------------------------------------
@pytest.mark.parametrize("c", (2, 3))
def test_grouped_repulsion_equals_the_full_one(c):
    rng = np.random.default_rng(c)
    pts = rng.normal(size=(97, c)).astype(np.float32)
    pts[0] = 0.0
    pts[1, 0] = -0.0  # a negative zero is its own bit pattern and the same position
    y = pts[rng.integers(0, 97, 2000)]
    Zr, R = to.repulsion(y)
    Zg, Rg = to.repulsion_grouped(y)
    assert Zg.dtype == np.int64 and Rg.dtype == np.int64 and np.array_equal(Zg, Zr) and np.array_equal(Rg, R)
    assert len(np.unique(y, axis=0)) == 97 and R.any()
    og = to.Graph(to.ring_graph(2000, offsets=(1, 7, 300)))
    assert to.gradient(og, y, 12.0, repulse=to.repulsion_grouped).tobytes() == to.gradient(og, y, 12.0).tobytes()
    lone = np.float32([[0.5, -1.0, 2.0][:c]])  # n = 1: no pair at all
    assert to.repulsion_grouped(lone)[0].tolist() == [0] and not to.repulsion_grouped(lone)[1].any()


def test_repulse_geometry():
    geom = to.repulse_geometry
    assert geom(11520) == (45, 45, 45, 256, 45)  # the largest n of one tile per workgroup
    assert geom(11521) == (46, 46, 45, 512, 23) and 11521 - 22 * 512 == 257
    assert geom(16385) == (65, 65, 32, 768, 22) and 16385 - 21 * 768 == 257
    assert geom(257) == (2, 2, 2, 256, 2)
    for n in (1, 2, 255, 256):
        assert geom(n) == (1, 1, 1, 256, 1)
    assert all(geom(n)[3] == 256 for n in (257, 2000, 5000, 11520)) and geom(20000)[3] == 1024
    for n in (1, 300, 11521, 16385, 20000, 10 ** 6, 1 << 30):  # the grid covers every position once, in whole tiles
        i_blocks, tiles, split, chunk, grid_y = geom(n)
        assert chunk % to.TILE == 0 and (grid_y - 1) * chunk < n <= grid_y * chunk and grid_y <= split <= 65535
    assert to.TILE_SIZES == (11520, 11521, 16385)


@pytest.mark.parametrize("c", (2, 3))
def test_tile_inputs_enter_their_branches(c):
    for n in to.TILE_SIZES:
        chunk = to.repulse_geometry(n)[3]
        tile_of = np.arange(n) // to.TILE
        y = {v: to.tile_positions(n, c, v) for v in to.TILE_VARIANTS}
        pts, inv = np.unique(y["drawn"], axis=0, return_inverse=True)
        assert len(pts) == 100
        counts = np.zeros((tile_of.max() + 1, 100), dtype=np.int64)
        np.add.at(counts, (tile_of, np.asarray(inv).reshape(-1)), 1)
        assert len(np.unique(counts, axis=0)) == len(counts)  # no two tiles hold the same counts
        last = y["lonely_last"]
        assert not (last[:-1] == last[-1]).all(axis=1).any() and np.array_equal(last[:-1], y["drawn"][:-1])
        if n % to.TILE == 1:
            assert tile_of[-1] != tile_of[-2] and (n - 1) % chunk == to.TILE  # the one cell of the last, partial tile
        # dropping that cell changes every other Zr
        assert (to.repulsion_grouped(last)[0][:-1] != to.repulsion_grouped(last[:-1])[0]).all()
        second = y["second_tile"]
        assert (second[256:512] == second[0]).all() and (chunk == 256 or 512 <= chunk)
        assert to.repulsion_grouped(second)[0][0] >= 256 << 32
        g = to.ring_graph(n)
        assert (np.diff(g.indptr) == 8).all() and (g != g.T).nnz == 0
        state = to.crafted_state(y["drawn"], scale=2.0 ** -10)
        assert len(np.unique(state[1].view(np.uint32))) == 8 and len(np.unique(state[2])) == 5


def test_row_graphs_sit_at_the_long_row_threshold():
    longest = {"star511": 511, "star512": 512, "star513": 513, "star768": 768, "two_centres": 600, "last_vertex": 600}
    for name, n_long in to.ROW_GRAPHS.items():
        g = to.row_graph(name)
        og = to.Graph(g)
        lengths = np.diff(og.indptr)
        assert lengths.max() == longest[name] and int((lengths > to.LONG_ROW).sum()) == n_long, name
        assert (g != g.T).nnz == 0 and g.has_sorted_indices
        w32 = g.data.astype(np.float32)
        tiny = np.finfo(np.float32).tiny
        assert w32.max() == 2.0 and (w32 == 2.0).sum() == 2 and (w32 == 0.0).sum() == 2  # each value and its mirror
        assert ((w32 > 0) & (w32 < tiny)).sum() == 2 and len(og.w) == g.nnz  # the stored 0 stays stored
        if name == "two_centres":
            assert sorted(lengths[lengths > to.LONG_ROW].tolist()) == [513, 600]
        if name == "last_vertex":
            assert lengths[-1] == 600 and lengths[:-1].max() == 1
    assert 768 % 256 == 0 and 768 % 512 != 0 and 600 % 256 != 0  # a long row's last round of 256 lanes is partial at 513, 600


def test_affinity_rows_enter_their_branches():
    """What the hand-built distances do in the oracle (kk = 15 carries the properties; the other kk the kinds)."""
    rows, e = to.affinity_scaled(15)
    assert e[0] == -62 and e[-1] == 62 and (np.diff(e) == 4).all() and (rows[:, 0] == 0).all()
    base = to.affinity_base(15)[None, :]
    assert np.array_equal(rows[e == 2], base * np.float32(4)) and 0 not in e
    for perplexity, last_up, first_down in ((5.0, -34, 34), (14.999, -38, 30)):
        beta, p = to.affinities(rows, perplexity)
        steps = to.affinities_steps(rows, perplexity)
        assert np.isfinite(p).all() and np.isfinite(beta).all()
        up, down = e <= last_up, e >= first_down
        assert (beta[up] == 2.0 ** 63).all() and (beta[down] == 2.0 ** -63).all()
        assert (steps[up | down] == -1).all() and (steps[~(up | down)] >= 0).all()
        mid = np.flatnonzero(~(up | down))
        b0, p0 = (a[0] for a in to.affinities(base, perplexity))
        assert np.array_equal(beta[mid], np.ldexp(b0, -2 * e[mid]))  # the shift is exact
        assert all(p[i].tobytes() == p0.tobytes() for i in mid)
        # the small end: every beta rel_r <= x = 2^63 2^2e 14 / 4, so e_r lies in [1 - x, 1] and p_r 15 within x of 1:
        # to rounding at e = -62 (x = 2^-59)
        x = np.ldexp(3.5, 63 + 2 * e[up])
        assert (np.abs(p[up] * 15 - 1).max(axis=1) <= x + 2.0 ** -50).all() and x[0] < 2.0 ** -59
        # the large end: beta rel_r >= x = 2^(2e - 63) / 4 for r >= 1, so p_0 >= 1 / (1 + 14 exp(-x)): x = 8 at e = 34
        x = np.ldexp(0.25, 2 * e[down] - 63)
        assert (p[down][:, 0] >= 1 / (1 + 14 * np.exp(-x)) - 1e-15).all() and (p[e >= 34][:, 0] > 0.995).all()
        big = e >= 40
        assert np.array_equal(p[big], np.eye(1, 15).repeat(big.sum(), axis=0))  # beta rel_1 >= 2^15: (1, 0, ...)
        if perplexity == 5.0:
            assert 2.0 < b0 < 4.0 and steps[e == -30][0] == 62  # bracketed only at beta = 2^62
    assert round(float(to.affinities(base, 14.999)[0][0]), 6) == 0.010691

    for kk in to.AFFINITY_KK:
        d, kinds = to.affinity_rows(kk, to.AFFINITY_N[-1])
        assert d.dtype == np.float32 and all(set(kinds[w:w + 64]) == set(to.AFFINITY_KINDS) for w in range(0, 960, 64))
        assert to.affinity_rows(kk, 257)[0].tobytes() == d[:257].tobytes()
        assert to.affinity_perplexities(kk) == {1: (0.999,), 2: (1.999,), 15: (5.0, 14.999), 63: (5.0, 62.999)}[kk]
        rel = d.astype(np.float64) ** 2
        rel -= rel[:, :1]
        for perplexity in to.affinity_perplexities(kk):
            beta, p = to.affinities(d, perplexity)
            steps = to.affinities_steps(d, perplexity)
            assert np.isfinite(p).all() and np.isfinite(beta).all() and (p >= 0).all()
            assert (steps[kinds == "flat"] == -2).all()
            if kk == 1:
                assert (steps == -2).all() and (beta == 1).all() and (p == 1).all()
                continue
            for w in range(0, 960, 64):  # a wavefront: flat rows, rows never bracketed at either end, late ones
                s, b = steps[w:w + 64], beta[w:w + 64]
                assert (s == -2).any() and (b == 2.0 ** 63).any() and (b == 2.0 ** -63).any() and (s >= 30).any()
            assert (steps >= 60).any() and (d[kinds == "d0_positive"][:, 0] > 0).all()
            assert (steps[kinds == "d0_positive"] >= 0).all()
            if kk >= 15:
                nine = kinds == "nine_zeros"
                assert (d[nine][:, :9] == 0).all() and (d[nine][:, 9] > 0).all()
                if perplexity == 5.0:  # nine neighbours tie at 0: the entropy never falls below log 9
                    assert (beta[nine] == 2.0 ** 63).all() and (p[nine][:, :9] == 1 / 9).all()
                    under = kinds == "underflow"
                    assert ((beta[:, None] * rel)[under][:, 7:] > 708).all() and (p[under][:, 7:] == 0).all()
                    assert (steps[under] >= 0).all()


@pytest.mark.parametrize("c", (2, 3))
def test_update_cases_enter_their_branches(c):
    floor = np.float32(0.01)
    g, state = to.update_case("crossed", c)
    og = to.Graph(g)
    y, u, gain = state
    assert y.shape == (300, c)
    for t in (249, 250, 251):
        gr = to.gradient(og, y, to.schedule(t)[0])
        combos = {(float(a), float(b).hex(), bool(s)) for a, b, s in zip(gain.ravel(), u.ravel(), (gr < 0).ravel())}
        assert len(combos) == 5 * 8 * 2 and (gr != 0).all()  # every gain x update x sign of the gradient
        new = to.iteration(og, *state, t)
        raw = np.where(u.astype(np.float64) * gr < 0, gain.astype(np.float64) + 0.2, gain.astype(np.float64) * 0.8)
        assert (raw < 0.01).any() and (new[2][raw < 0.01] == floor).all() and (new[2] >= floor).all()
        assert float(np.float32(0.0125)) * 0.8 >= 0.01 > float(np.float32(0.012)) * 0.8  # on either side of the floor
        zero = (u.astype(np.float64) * gr == 0)
        k = np.arange(y.size) % 8
        assert np.array_equal(zero, u == 0) and zero.sum() == (k < 2).sum() and np.signbit(u[zero]).sum() == (k == 1).sum()
        assert all(np.isfinite(a).all() for a in new)

    g, state = to.update_case("zero_gradient", c)
    og = to.Graph(g)
    assert g.nnz == 0 and not to.gradient(og, state[0], 12.0).any() and (state[1] != 0).any()
    new = to.iteration(og, *state, 0)
    assert new[1].tobytes() == (state[1] * np.float32(0.5)).tobytes() and np.signbit(new[1]).sum() == state[1].size // 2
    assert np.array_equal(new[2], np.maximum((state[2].astype(np.float64) * 0.8).astype(np.float32), floor))

    one = (sp.csr_matrix((1, 1)), to.crafted_state(np.ones((1, c), dtype=np.float32)))
    for g, state in (one, to.update_case("far_line", c)):
        Zr, R = to.repulsion(state[0])
        assert to.normaliser(Zr) == 0.0 and not Zr.any() and not R.any()
        gr = to.gradient(to.Graph(g), state[0], 12.0)
        assert np.isfinite(gr).all() and (gr.any() or g.nnz == 0)
    d = np.diff(to.update_case("far_line", c)[1][0][:, 0].astype(np.float64))
    assert (1.0 / (1.0 + d.min() ** 2) < 2.0 ** -33) and len(d) == 299

    g, state = to.update_case("huge", c)
    Zr, R, _ = to.repulsion(state[0], return_abs=True)
    y64 = state[0].astype(np.float64)
    d2 = ((y64[:, None, :] - y64[None, :, :]) ** 2).sum(axis=2)
    assert d2.max() >= 1e11 * c and to.normaliser(Zr) > 0
    terms = np.rint(4294967296.0 / (1.0 + d2[~np.eye(300, dtype=bool)]))
    assert (terms <= 1).mean() > 0.5 and (terms == 0).any() and (terms == 1).any()

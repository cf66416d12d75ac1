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

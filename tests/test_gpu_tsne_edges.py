"""GPU tests (``-m gpu``): tl.tsne at its tile, row-length, bisection and gain limits, against the numpy oracle of
DESIGN.md 4.12 (tests/_tsne_oracle.py).  The inputs are the builders of the oracle file; that the oracle itself enters
the branch each of them is for is asserted on the CPU in tests/test_tsne_oracle.py.  Every comparison is ``tobytes()``
equality.

What test_gpu_tsne.py does not enter: a second round of the tile loop of k_ts_repulse (chunk > 256 needs n > 11 520),
a chunk of one full tile and a partial one, rows of 511 to 513 entries (the split between a wavefront and a workgroup in
k_ts_step), a bisection that never brackets or brackets after 60 doublings, kk = 1, 2 and 63, a gain at its floor,
u g = 0 with u = -0, and Z = 0."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _tsne_oracle as to

pytestmark = pytest.mark.gpu


def _device(g):
    import torch

    g = sp.csr_matrix(g)
    g.sort_indices()
    return (torch.from_numpy(g.indptr.astype(np.int64)).cuda(), torch.from_numpy(g.indices.astype(np.int32)).cuda(),
            torch.from_numpy(g.data.astype(np.float32)).cuda())


def _gpu(dev, state, t0, t1):
    import torch

    from infercnvpy_amd import _engine

    y, u, gain = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in state)
    _engine.tsne_iterations(*dev, y, u, gain, iter_begin=t0, iter_end=t1)
    return y.cpu().numpy(), u.cpu().numpy(), gain.cpu().numpy()


def _assert_same(got, ref, what):
    for name, r, g in zip(("y", "u", "gain"), ref, got):
        bad = np.flatnonzero((g.view(np.uint32) != r.view(np.uint32)).any(axis=1))
        assert g.tobytes() == r.tobytes(), (what, name, len(bad), bad[:8].tolist(), g[bad[:3]].tolist(), r[bad[:3]].tolist())


def _check(og, dev, state, t, what, repulse=to.repulsion):
    ref = to.iteration(og, *state, t, grad=to.gradient(og, state[0], to.schedule(t)[0], repulse=repulse))
    _assert_same(_gpu(dev, state, t, t + 1), ref, what)
    return ref


@functools.lru_cache(maxsize=None)
def _ring(n):
    g = to.ring_graph(n)
    return to.Graph(g), _device(g)


# ---- a. the tile loop of k_ts_repulse ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (2, 3))
@pytest.mark.parametrize("n", to.TILE_SIZES)
def test_tiles(n, c):
    """One iteration from start(y) and one from a crafted (u, gain), for the three kinds of positions; then [0, 2) in
    one call against two calls of one iteration (the tickets and the other accumulator set between iterations)."""
    og, dev = _ring(n)
    for variant in to.TILE_VARIANTS:
        y = to.tile_positions(n, c, variant)
        first = _check(og, dev, to.start(y), 0, (n, c, variant, "start"), to.repulsion_grouped)
        _check(og, dev, to.crafted_state(y, scale=2.0 ** -10), 250, (n, c, variant, "crafted"), to.repulsion_grouped)
        two = _gpu(dev, to.start(y), 0, 2)
        _assert_same(two, _gpu(dev, first, 1, 2), (n, c, variant, "[0, 2)"))
        assert len(np.unique(first[0], axis=0)) > 1000  # the cells have left their 100 points


def test_tiles_second_iteration_equals_the_full_oracle():
    """The one call of the full O(n^2) oracle at a size with two tiles per workgroup: iteration 1 of [0, 2)."""
    n, c = 11521, 2
    og, dev = _ring(n)
    y = to.tile_positions(n, c, "lonely_last")
    first = to.iteration(og, *to.start(y), 0, grad=to.gradient(og, y, 12.0, repulse=to.repulsion_grouped))
    _assert_same(_gpu(dev, to.start(y), 0, 2), to.iteration(og, *first, 1), (n, c, "second iteration"))


# ---- b. the short / long row switch of k_ts_step -----------------------------------------------------------------------
@pytest.mark.parametrize("c", (2, 3))
@pytest.mark.parametrize("name", tuple(to.ROW_GRAPHS))
def test_row_lengths(name, c):
    g = to.row_graph(name)
    og, dev = to.Graph(g), _device(g)
    assert dev[2].numel() == g.nnz and int((dev[2] == 0).sum()) == 2  # the stored zeros reach the device
    rng = np.random.default_rng(c)
    y = rng.normal(size=(og.n, c)).astype(np.float32)
    for t in (0, 250):
        _check(og, dev, to.start(y), t, (name, c, t, "start"))
        _check(og, dev, to.crafted_state(y), t, (name, c, t, "crafted"))


# ---- c. the bisection of k_ts_affinity on hand-built distances ---------------------------------------------------------
@pytest.mark.parametrize("n", to.AFFINITY_N)
@pytest.mark.parametrize("kk", to.AFFINITY_KK)
def test_affinities_of_hand_built_distances(kk, n):
    import torch

    from infercnvpy_amd import _engine

    d, kinds = to.affinity_rows(kk, n)
    dist = torch.from_numpy(d).cuda()
    for perplexity in to.affinity_perplexities(kk):
        beta, p = to.affinities(d, perplexity)
        d_beta, d_p = (a.cpu().numpy() for a in _engine.tsne_affinities(dist, perplexity))
        bad = np.flatnonzero(d_beta.view(np.uint64) != beta.view(np.uint64))
        assert d_beta.tobytes() == beta.tobytes(), (kk, n, perplexity, len(bad), bad[:5].tolist(), kinds[bad[:5]].tolist(),
                                                    d_beta[bad[:5]].tolist(), beta[bad[:5]].tolist())
        bad = np.flatnonzero((d_p.view(np.uint64) != p.view(np.uint64)).any(axis=1))
        assert d_p.tobytes() == p.tobytes(), (kk, n, perplexity, len(bad), bad[:5].tolist(), kinds[bad[:5]].tolist())


# ---- d. the update rule on crafted states ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (2, 3))
@pytest.mark.parametrize("name", to.UPDATE_CASES)
def test_update_rule_on_crafted_states(name, c):
    g, state = to.update_case(name, c)
    og, dev = to.Graph(g), _device(g)
    for t in (249, 250, 251):
        _check(og, dev, state, t, (name, c, t))


@pytest.mark.parametrize("c", (2, 3))
def test_one_cell(c):
    """n = 1: no pair, Z = 0, the gradient is 0 and only the momentum and the gain's decay act."""
    g = sp.csr_matrix((1, 1), dtype=np.float64)
    og, dev = to.Graph(g), _device(g)
    for k in range(8):
        y, u, gain = to.crafted_state(np.ones((8, c), dtype=np.float32))
        state = tuple(np.ascontiguousarray(a[k:k + 1]) for a in (y, u, gain))
        for t in (0, 250):
            ref = _check(og, dev, state, t, (c, k, t))
            assert ref[1].tobytes() == (state[1] * np.float32(to.schedule(t)[1])).tobytes()

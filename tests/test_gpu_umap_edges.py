"""tl.umap at its row-length, activity, sampling and clip limits ("Edge pass").  Every comparison is ONE
device epoch against the numpy oracle from the same snapshot, within the derived bound of ``_umap_checks.check_epoch``
(spacing(|ref|) + m 2^-32; rows without a contribution bit-equal to the input).  tests/test_umap_oracle.py asserts on
the CPU that the oracle enters the branch each builder is for, and that the bound cannot hide a lost entry."""
import numpy as np
import pytest

import _umap_oracle as uo
from _umap_checks import A, B, check_epoch, coincident, device, gpu_epochs

pytestmark = pytest.mark.gpu
N30 = 30
EDGE_EPOCHS = (1, 2, 7, 15, 29)
SETTINGS = ((2, 0), (3, 1))  # (n_components, random_state)
SCALE = np.float32(0.01)
_cache = {}


def _graph(name, *args):
    key = (name,) + args
    if key not in _cache:
        g = getattr(uo, name)(*args)
        _cache[key] = (g, uo.Graph(g))
    return _cache[key]


def _snapshots(og, y0):
    return (("random", y0), ("scaled", y0 * SCALE), ("coincident", coincident(og, y0)))


# ---- 1. short rows of more than one chunk whose ballots are partial; rows on both sides of the split -------------------
@pytest.mark.parametrize("c, seed", SETTINGS)
@pytest.mark.parametrize("leaves", (1030, 1031))  # n = 1044 (a multiple of 4) and 1045 (the last workgroup has one row)
def test_chunked_compaction(leaves, c, seed):
    g, og = _graph("hubs_mixed", uo.HUBS, leaves)
    dev = device(g)
    y0 = uo.random_init(og.n, c, seed)
    for t in EDGE_EPOCHS:
        for name, y in _snapshots(og, y0):
            check_epoch(og, dev, y, t, N30, seed, (leaves, c, seed, t, name))
        if t > 1:  # the device's own trajectory from the random start
            y = gpu_epochs(dev, y0, 0, t, N30, seed)
            assert np.isfinite(y).all()
            check_epoch(og, dev, y, t, N30, seed, (leaves, c, seed, t, "trajectory"))


# ---- 2. hundreds of long rows next to hundreds of short ones, all with mixed activity ----------------------------------
@pytest.mark.parametrize("c, seed", SETTINGS)
def test_rows_at_the_split_and_many_long_rows(c, seed):
    g, og = _graph("split_mixed")
    dev = device(g)
    y0 = uo.random_init(og.n, c, seed)
    cases = [(1, "random", y0), (7, "random", y0), (29, "random", y0), (7, "scaled", y0 * SCALE),
             (1, "coincident", coincident(og, y0)), (29, "trajectory", gpu_epochs(dev, y0, 0, 29, N30, seed))]
    for t, name, y in cases:
        got = check_epoch(og, dev, y, t, N30, seed, (c, seed, t, name))
        # the list of the long rows is filled in another order in every call
        assert gpu_epochs(dev, y, t, t + 1, N30, seed).tobytes() == got.tobytes(), (c, seed, t, name)
    whole = gpu_epochs(dev, y0, 0, N30, N30, seed)
    assert gpu_epochs(dev, y0, 0, N30, N30, seed).tobytes() == whole.tobytes() and np.isfinite(whole).all()


# ---- 3. negative_sample_rate at 1, at its limit 64, and beyond ---------------------------------------------------------
@pytest.mark.parametrize("c, seed", SETTINGS)
@pytest.mark.parametrize("rate", (1, 64))
def test_sample_rate_limits(rate, c, seed):
    g, og = _graph("hubs_mixed", uo.HUBS, 1030)
    dev = device(g)
    y0 = uo.random_init(og.n, c, seed)
    for t in (1, 7, 29):
        got = check_epoch(og, dev, y0, t, N30, seed, (rate, c, seed, t), negative_sample_rate=rate)
        assert not np.array_equal(got, y0)
    check_epoch(og, dev, coincident(og, y0), 7, N30, seed, (rate, c, seed, "d2 == 0"), negative_sample_rate=rate)
    check_epoch(og, dev, y0 * SCALE, 7, N30, seed, (rate, c, seed, "scaled"), negative_sample_rate=rate)


def test_sample_rate_beyond_the_limit_is_an_error():
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    g, og = _graph("hubs_mixed", uo.HUBS, 1030)
    dev = device(g)
    y0 = uo.random_init(og.n, 2, 0)
    for rate in (65, -1):
        yd = torch.from_numpy(y0).cuda()
        with pytest.raises(ValueError, match="umap_epochs"):
            _engine.umap_epochs(*dev, yd, a=A, b=B, n_epochs=N30, epoch_begin=7, epoch_end=8, negative_sample_rate=rate)
        assert yd.cpu().numpy().tobytes() == y0.tobytes()
        with pytest.raises(ValueError, match="negative_sample_rate"):
            cnv.tl.umap(None, adjacency=dev, inplace=False, init_pos="random", negative_sample_rate=rate)


# ---- 4. both clips, of the attraction (doubled: +-8) and of the repulsion (+-4) ----------------------------------------
@pytest.mark.parametrize("c, seed", SETTINGS)
@pytest.mark.parametrize("a, b", ((100.0, 1.0), (30.0, 0.4)))
def test_clips(a, b, c, seed):
    g, og = _graph("hubs_mixed", uo.HUBS, 1030)
    dev = device(g)
    y0 = uo.random_init(og.n, c, seed)
    _, q = uo.contributions(og, y0 * SCALE, 7, n_epochs=N30, a=a, b=b, seed=seed)
    assert all((q == v * 2 ** 32).any() for v in (-8, -4, 4, 8))
    for t in EDGE_EPOCHS:
        for name, y in _snapshots(og, y0):
            check_epoch(og, dev, y, t, N30, seed, (a, b, c, seed, t, name), a=a, b=b)


# ---- 5. the limits of the schedule -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_epochs", (32, 30))
def test_schedule_thresholds(n_epochs):
    import infercnvpy_amd as cnv

    g, og = _graph("threshold_weights", n_epochs)
    dev = device(g)
    assert np.signbit(dev[2].cpu().numpy()).sum() == 2  # -0.0 reaches the device as it is
    for c, seed in SETTINGS:
        y0 = uo.random_init(og.n, c, seed)
        for t in range(n_epochs):
            got = check_epoch(og, dev, y0, t, n_epochs, seed, (n_epochs, c, seed, t))
            # the leaves at, above and below the threshold, the two zeros: never moved
            assert got[2:7].tobytes() == y0[2:7].tobytes()
        y, info = cnv.tl.umap(None, adjacency=dev, inplace=False, init_pos="random", random_state=seed, n_components=c,
                              maxiter=n_epochs, return_info=True)
        assert info["n_fire"] == int(og.fires(n_epochs).sum()) == 16
        assert y.tobytes() == gpu_epochs(dev, y0, 0, n_epochs, n_epochs, seed, a=info["a"], b=info["b"]).tobytes()
        assert y[2:7].tobytes() == y0[2:7].tobytes() and not np.array_equal(y[1], y0[1])


def test_nothing_to_do_returns_the_positions_bit_for_bit():
    import infercnvpy_amd as cnv

    g, og = _graph("zero_weights")
    dev = device(g)
    hubs = device(_graph("hubs_mixed", uo.HUBS, 1030)[0])
    for c, seed in SETTINGS:
        y0 = uo.random_init(og.n, c, seed)
        assert gpu_epochs(dev, y0, 0, N30, N30, seed).tobytes() == y0.tobytes()  # w_max = 0
        for t in (1, 7, 29):
            check_epoch(og, dev, y0, t, N30, seed, ("zero", c, seed, t))
        y, info = cnv.tl.umap(None, adjacency=dev, inplace=False, init_pos="random", random_state=seed, n_components=c,
                              maxiter=N30, return_info=True)
        assert info["n_fire"] == 0 and y.tobytes() == y0.tobytes()
        y1 = uo.random_init(1044, c, seed)
        assert gpu_epochs(hubs, y1, 0, 1, 1, seed).tobytes() == y1.tobytes()  # n_epochs = 1: only epoch 0
        for t in (0, 7, N30):
            assert gpu_epochs(hubs, y1, t, t, N30, seed).tobytes() == y1.tobytes()  # epoch_begin == epoch_end
        assert gpu_epochs(hubs, y1, 7, 8, N30, seed).tobytes() != y1.tobytes()


# ---- 6. validation: device tuples, because the host path canonicalises -------------------------------------------------
def test_device_validation_flags():
    import torch

    import infercnvpy_amd as cnv

    g = uo.threshold_weights(30)
    n = g.shape[0]
    indptr, indices, data = device(g)
    row0 = slice(int(g.indptr[0]), int(g.indptr[1]))  # the centre: 8 ascending columns

    def run(ind=indices, dat=data):
        return cnv.tl.umap(None, adjacency=(indptr, ind, dat), inplace=False, init_pos="random", maxiter=5)

    def with_columns(at, values):
        ind = indices.clone()
        ind[at] = torch.tensor(values, dtype=torch.int32, device="cuda")
        return ind

    assert np.isfinite(run()).all()  # as it is (with its -0.0) the graph is accepted
    assert np.isfinite(run(dat=torch.where(data == 0, -data, data))).all()
    last, first = row0.stop - 1, row0.start
    swapped = [int(g.indices[first + 1]), int(g.indices[first])]
    ulp = data.clone()
    ulp[first] = float(np.nextafter(g.data[first], np.float32(2.0)))  # its mirror keeps the value
    nan = data.clone()
    nan[first] = float("nan")
    for what, kw in (("out of range", dict(ind=with_columns([last], [n]))),
                     ("out of range", dict(ind=with_columns([first], [-1]))),
                     ("sorted", dict(ind=with_columns([first, first + 1], swapped))),
                     ("sorted", dict(ind=with_columns([first + 1], [int(g.indices[first])]))),
                     ("symmetric", dict(dat=ulp)),
                     ("finite", dict(dat=nan))):
        with pytest.raises(ValueError, match=what):
            run(**kw)

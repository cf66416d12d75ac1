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


# ---- the edge builders: the oracle alone reaches every branch that tests/test_gpu_umap_edges.py relies on -------------
N30 = 30
EDGE_EPOCHS = (1, 2, 7, 15, 29)
SETTINGS = ((2, 0), (3, 1))  # (n_components, random_state), as in the GPU tests


@pytest.fixture(scope="module", params=(1030, 1031))
def hubs(request):
    g = uo.hubs_mixed(leaves=request.param)
    return g, uo.Graph(g), uo.hub_rows(g, request.param)


@pytest.fixture(scope="module")
def split():
    g = uo.split_mixed()
    return g, uo.Graph(g)


def test_hubs_mixed_is_what_it_says(hubs):
    g, og, rows = hubs
    leaves = rows[0]
    assert og.n == leaves + 14 and len(og.w) == 10_512 + 2 * (leaves - 1030) and og.n % 4 == leaves - 1030
    assert tuple(np.diff(og.indptr)[rows]) == uo.HUBS and og.w_max == 1.0
    assert (g != g.T).nnz == 0 and np.array_equal(og.w * 64, np.rint(og.w * 64))
    assert 50 < (og.w == 0).sum() < 300  # the zeros are stored
    for v in rows:
        assert np.array_equal(og.indices[og.indptr[v]:og.indptr[v + 1]], np.arange(np.diff(og.indptr)[v]))


def test_hub_chunks_mix_active_and_inactive_entries(hubs):
    _, og, rows = hubs
    short = [v for v in rows if np.diff(og.indptr)[v] <= uo.LDS_ROW]
    assert len(short) == 11
    single_seen = set()
    for t in (2, 7, 15, 29):
        for v in short:
            na, size = uo.chunk_counts(og, v, t, N30)
            assert ((na > 0) & (na < size))[size >= 2].all(), (t, v, na)  # a chunk of one entry cannot mix
            if size[-1] == 1 and na[-1] == 1 and na[:-1].sum() % uo.CHUNK != 0:
                single_seen.add(v)
    # the rows of 65, 129 and 193 entries end in a chunk of one entry: it is written behind a partial carry
    assert single_seen == {v for v in short if np.diff(og.indptr)[v] % uo.CHUNK == 1} and len(single_seen) == 3
    # epoch 1: only the weights 1 are active
    counts = {int(np.diff(og.indptr)[v]): uo.chunk_counts(og, v, 1, N30)[0] for v in short}
    assert counts[127].sum() == 0  # a non-empty row that copies its position
    assert sum(int((na == 0).sum()) for na in counts.values()) >= 5  # chunks that are wholly inactive
    assert any(((na[:-1] == 0) & (np.cumsum(na[::-1])[::-1][1:] > 0)).any() for na in counts.values())
    assert counts[512][0] == 0 and counts[512][1] > 0  # ... ahead of a chunk that is not


def test_hub_rows_above_the_split_have_mixed_activity(hubs):
    _, og, rows = hubs
    long_rows = [v for v in rows if np.diff(og.indptr)[v] > uo.LDS_ROW]
    assert [int(np.diff(og.indptr)[v]) for v in long_rows] == [513, 514, 1025]
    for t in EDGE_EPOCHS:
        for v in long_rows:
            na, size = uo.chunk_counts(og, v, t, N30)
            assert 0 < na.sum() < size.sum()


def test_split_mixed_is_what_it_says(split):
    g, og = split
    length = np.diff(og.indptr)
    assert og.n == 1539 and len(og.w) == 787_976 and (g != g.T).nnz == 0 and og.w_max == 1.0
    assert set(length) == {511, 512, 513, 514}
    assert (length > uo.LDS_ROW).sum() >= 500 and (length <= uo.LDS_ROW).sum() >= 500
    assert np.array_equal(og.w * 8, np.rint(og.w * 8)) and (og.w == 0).sum() > 10_000
    for t in (1, 7, 29):
        na = np.bincount(og.rows[og.active(t, N30)], minlength=og.n)
        assert ((na > 0) & (na < length)).all(), t  # every row, whatever its length, has mixed activity


def _clip_counts(q):
    return {s * k: int((q == s * k * 2 ** 32).sum()) for k in (4, 8) for s in (-1, 1)}


def test_contributions_reach_all_four_clip_values(hubs):
    _, og, _ = hubs
    for c, seed in SETTINGS:
        y = uo.random_init(og.n, c, seed)
        _, q = uo.contributions(og, y * np.float32(0.01), 7, n_epochs=N30, a=100.0, b=1.0, seed=seed)
        counts = _clip_counts(q)
        assert min(counts.values()) >= 1000, counts
        assert np.abs(q).max() == 8 * 2 ** 32
        _, q = uo.contributions(og, y * np.float32(0.01), 7, n_epochs=N30, a=30.0, b=0.4, seed=seed)
        assert min(_clip_counts(q).values()) > 0
        # with the default (a, b) the attraction stays below the clip (its maximum over d is about 1.1): only +-4
        for scale in (1.0, 0.01):
            _, q = uo.contributions(og, y * np.float32(scale), 7, n_epochs=N30, a=A, b=B, seed=seed)
            counts = _clip_counts(q)
            assert counts[-8] == counts[8] == 0 and np.abs(q).max() == 4 * 2 ** 32, counts
            assert counts[-4] + counts[4] > 0, counts


@pytest.mark.parametrize("n_epochs", (32, 30))
def test_threshold_weights_sit_on_the_limits_of_the_schedule(n_epochs):
    g = uo.threshold_weights(n_epochs)
    og = uo.Graph(g)
    names = list(uo.threshold_values(n_epochs))
    val = uo.threshold_values(n_epochs)
    assert og.w_max == 1.0 and (g != g.T).nnz == 0 and g.data.dtype == np.float32
    exact = float(val["at"]) == 1.0 / n_epochs  # float32(1 / 32) is 1 / 32; float32(1 / 30) lies above 1 / 30
    assert exact == (n_epochs == 32) and float(val["at"]) >= 1.0 / n_epochs
    assert float(val["below"]) < 1.0 / n_epochs < float(val["above"]) and float(val["subnormal"]) == 2.0 ** -149
    e = {name: int(og.indptr[0]) + q for q, name in enumerate(names)}  # the centre's row holds them in this order
    assert np.array_equal(og.w[[e[k] for k in names]], [float(val[k]) for k in names])
    assert np.signbit(g.data[e["minus_zero"]]) and not np.signbit(g.data[e["zero"]])
    fires = og.fires(n_epochs)
    assert [bool(fires[e[k]]) for k in names] == [True, True, True, False, False, False, True, False]
    assert fires.sum() == 2 * (4 + 4)
    seen = np.zeros(len(og.w), dtype=np.int64)
    for t in range(n_epochs):
        seen[og.active(t, n_epochs)] += 1
    # the boundary weight fires, but its period is n_epochs (up to float32's rounding): not before the schedule ends
    assert seen[e["at"]] == 0 and seen[e["above"]] == 0 and seen[e["below"]] == 0
    assert seen[e["zero"]] == seen[e["minus_zero"]] == seen[e["subnormal"]] == 0
    assert seen[e["one"]] == n_epochs - 1 and seen[e["third"]] == (n_epochs - 1) // 3
    # rows with a firing and a never-firing entry, and rows whose only entry never becomes active
    length = np.diff(og.indptr)
    per_row = np.bincount(og.rows, weights=seen, minlength=og.n)
    assert ((per_row == 0) & (length > 0)).sum() == 5 and (per_row[length == 2] > 0).all()


def test_zero_weights_never_fire():
    g = uo.zero_weights()
    og = uo.Graph(g)
    assert len(og.w) == 40 and og.w_max == 0.0 and np.signbit(g.data).sum() == 20 and not g.data.any()
    assert not og.fires(N30).any() and all(len(og.active(t, N30)) == 0 for t in range(N30))
    y = uo.random_init(og.n, 2, 0)
    new, m = uo.epoch(og, y, 7, n_epochs=N30, a=A, b=B)
    assert new.tobytes() == y.tobytes() and not m.any()


def test_negative_samples_hit_the_row_itself_and_coincident_points(hubs):
    from _umap_checks import coincident

    _, og, _ = hubs
    for c, seed in SETTINGS:
        y = coincident(og, uo.random_init(og.n, c, seed))
        own = other = 0
        for t in EDGE_EPOCHS:
            i, k, d2 = uo.negatives(og, y, t, n_epochs=N30, seed=seed)
            own += int((k == i).sum())
            other += int(((k != i) & (d2 == 0)).sum())
        assert own > 0 and other > 0, (c, seed, own, other)


def _moved(og, y, t, seed, drop, scale_kw):
    full, m = uo.epoch(og, y, t, seed=seed, **scale_kw)
    less, _ = uo.epoch(og, y, t, seed=seed, drop=drop, **scale_kw)
    return (np.abs(full.astype(np.float64) - less.astype(np.float64)) > uo.tolerance(full, m)).any(axis=1)


@pytest.mark.parametrize("kw, epochs", ((dict(a=A, b=B), EDGE_EPOCHS), (dict(a=100.0, b=1.0), EDGE_EPOCHS),
                                        (dict(a=A, b=B, negative_sample_rate=1), (1, 7)),
                                        (dict(a=A, b=B, negative_sample_rate=64), (7,))),
                         ids=("default", "clipped", "r1", "r64"))
def test_the_tolerance_cannot_hide_a_lost_entry_at_a_chunk_boundary(hubs, kw, epochs):
    """Drop ONE active entry of a hub row from the oracle: the one at the compacted position 0, 63, 64 or the last one
    (rows up to 512 entries), the first or the last (longer rows).  Rows are independent, so one oracle call drops the
    entry of that position from every hub row at once.  Each row then moves by more than the tolerance of a
    comparison: a kernel that loses, doubles or misplaces an entry across a ballot cannot pass."""
    _, og, rows = hubs
    length = np.diff(og.indptr)
    for c, seed in SETTINGS:
        y0 = uo.random_init(og.n, c, seed)
        for scale in (1.0, 0.01):
            y = y0 * np.float32(scale)
            for t in epochs:
                act = og.active(t, N30)
                per_row = {v: act[og.rows[act] == v] for v in rows}
                for pos in (0, 63, 64, -1):
                    if pos >= 0 and length.max() > uo.LDS_ROW:
                        who = [v for v in rows if len(per_row[v]) > pos and (length[v] <= uo.LDS_ROW or pos == 0)]
                    else:
                        who = [v for v in rows if len(per_row[v]) > 0]
                    if not who:
                        continue
                    drop = np.array([per_row[v][pos] for v in who])
                    moved = _moved(og, y, t, seed, drop, dict(n_epochs=N30, **kw))
                    assert moved[who].all(), (c, seed, scale, t, pos, [int(length[v]) for v in who if not moved[v]])
                    assert moved.sum() == len(who)  # and no other row


def test_the_tolerance_cannot_hide_a_lost_entry_of_split_mixed(split):
    _, og = split
    y = uo.random_init(og.n, 2, 0)
    act = og.active(7, N30)
    first = act[np.unique(og.rows[act], return_index=True)[1]]
    last = act[len(act) - 1 - np.unique(og.rows[act][::-1], return_index=True)[1]]
    for drop in (first, last):
        assert _moved(og, y, 7, 0, drop, dict(n_epochs=N30, a=A, b=B)).all()

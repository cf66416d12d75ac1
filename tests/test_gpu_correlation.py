"""tl.cnv_correlation and tl.cnv_signal on the GPU equal the oracle of DESIGN.md 4.18 (tests/_correlation_oracle.py) on the
float64 bytes: the two entry points for every group width, row length and shape at which the kernel takes another path,
every kind of input, and the public functions in their three modes on the planted tumour / normal case."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _correlation_oracle as co
import _pseudobulk_oracle as pb

pytestmark = pytest.mark.gpu

# lanes per row: 1 (no profile), 8 (1, 2, 3 and 5 profiles: some lanes have none), 16, 32 and 64; above 64 profiles tiles
# of 64 (65: one lane of the second tile, 130: three tiles, 300 and 520: five and nine)
GROUPS = [0, 1, 2, 3, 5, 9, 17, 63, 64, 65, 130, 300, 520]
ROWS = [1, 5, 67]                          # 67 rows leave the last wavefront partly filled for every GP below 64
WINDOWS = [1, 2, 63, 64, 65, 270]


def matrix(n, w, seed, dtype=np.float64):
    """A canonical CSR matrix of float32 numbers whose rows have 0, 1, 64, 65 and W stored entries (as far as W goes) and
    random lengths after that, with stored 0.0 and -0.0 among the entries."""
    rng = np.random.default_rng(seed)
    edges = [min(v, w) for v in (0, 1, 64, 65, w)]
    lengths = edges + rng.integers(0, w + 1, size=n - 5).tolist() if n >= 5 else [edges[(seed + i) % 5] for i in range(n)]
    rng.shuffle(lengths)
    dense = np.zeros((n, w))
    stored = np.zeros((n, w), dtype=bool)
    for i, length in enumerate(lengths):
        stored[i, rng.choice(w, size=length, replace=False)] = True
    dense[stored] = rng.normal(0.0, 0.5, int(stored.sum())).astype(np.float32)
    zero = stored & (rng.random((n, w)) < 0.05)
    dense[zero] = 0.0
    cols = [np.flatnonzero(stored[i]) for i in range(n)]
    data = np.concatenate([dense[i, c] for i, c in enumerate(cols)] + [np.zeros(0)])
    data[(data == 0) & (np.arange(data.shape[0]) % 2 == 1)] = -0.0
    indptr = np.concatenate([[0], np.cumsum([c.shape[0] for c in cols])])
    x = sp.csr_matrix((data.astype(dtype), np.concatenate(cols + [np.zeros(0, dtype=np.int64)]).astype(np.int32), indptr),
                      shape=(n, w))
    assert x.has_canonical_format
    return x


def profiles(g, w, seed):
    """G profiles, the second of them constant."""
    p = np.random.default_rng(seed).normal(0.0, 0.3, (g, w))
    if g >= 2:
        p[1] = 0.75
    return p


def run_entries(x, p):
    """dict(A, B, signal, r, best_r, best_g, flags) of the two entry points for any kind of input, as host arrays."""
    from infercnvpy_amd import _engine
    from infercnvpy_amd.tl._correlation import centre_profiles

    dm = _engine.matrix_input(x, "test")
    if p.shape[0]:
        a, b, signal, r, flags = _engine.profile_corr(dm, *centre_profiles(p))
    else:
        a, b, signal, r, flags = _engine.profile_corr(dm)
    best_r, best_g = _engine.profile_corr_best(r)
    got = {k: v.cpu().numpy() for k, v in (("A", a), ("B", b), ("signal", signal), ("r", r), ("best_r", best_r),
                                          ("best_g", best_g))}
    got["flags"] = int(flags.item())
    return got


def assert_equal(got, want, what):
    for k in ("A", "B", "signal", "r", "best_r"):
        assert got[k].dtype == np.float64 and co.same_bytes(got[k], want[k]), (what, k)
    assert got["best_g"].dtype == np.int32 and np.array_equal(got["best_g"], want["best_g"]), what


# ---- the entry points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GROUPS)
def test_every_group_width_and_shape_gives_the_oracles_bytes(g):
    for n in ROWS:
        for w in WINDOWS:
            x, p = matrix(n, w, 7 * n + w), profiles(g, w, g + w)
            got = run_entries(x, p)
            assert got["flags"] == 0 and got["r"].shape == (n, g)
            assert_equal(got, co.correlate(x, p), (n, w, g))


@functools.lru_cache(maxsize=None)
def kinds_case():
    x = matrix(67, 270, 3)
    lengths = np.diff(x.indptr)
    assert {0, 1, 64, 65, 270} <= set(lengths.tolist()) and (x.data == 0).any() and np.signbit(x.data[x.data == 0]).any()
    out = {}
    for g in (5, 65):
        p = profiles(g, 270, g)
        want = co.correlate(x, p)
        assert np.isnan(want["r"][:, 1]).all() and (want["best_g"] >= 0).sum() >= 60 and (want["best_g"] == -1).any()
        out[g] = (p, want)
    return x, out


def _inputs(x):
    import torch

    import infercnvpy_amd as cnv

    def packed(tail):
        pad_i = torch.full((tail,), 2 ** 30, dtype=torch.int32)  # (never read: a column far outside the matrix, a NaN)
        pad_v = torch.full((tail,), float("nan"), dtype=torch.float64)
        return cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                             torch.cat([torch.from_numpy(x.indices.astype(np.int32)), pad_i]).cuda(),
                             torch.cat([torch.from_numpy(x.data), pad_v]).cuda(), x.shape[1])

    dense = x.toarray()
    return {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_c": dense,
            "dense_f": np.asfortranarray(dense), "dense_float32": dense.astype(np.float32),
            "cuda_float64": torch.from_numpy(dense).cuda(), "cuda_float32": torch.from_numpy(dense.astype(np.float32)).cuda(),
            "packed_csr": packed(0), "packed_csr_with_a_tail": packed(37)}


@pytest.mark.parametrize("g", [5, 65])
def test_every_input_kind_gives_the_oracles_bytes(g):
    x, cases = kinds_case()
    p, want = cases[g]
    for name, form in _inputs(x).items():
        got = run_entries(form, p)
        assert got["flags"] == 0, name
        assert_equal(got, want, name)


def test_a_non_finite_stored_value_sets_the_flag_and_nothing_else_breaks():
    x = matrix(67, 65, 5)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y.data[y.data.shape[0] // 2] = bad
        assert run_entries(y, profiles(3, 65, 1))["flags"] == 1
        assert run_entries(y.toarray(), profiles(0, 65, 1))["flags"] == 1
    assert run_entries(x, profiles(3, 65, 1))["flags"] == 0


# ---- the public functions ------------------------------------------------------------------------------------------------------
def _adata(x, clone=None):
    from infercnvpy_amd._compat import SimpleAnnData

    obs = pd.DataFrame(index=[f"cell{i}" for i in range(x.shape[0])])
    if clone is not None:
        obs["clone"] = pd.Categorical.from_codes(clone, categories=["clone0", "clone1", "clone2"])
    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32), obs=obs)
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 140}}
    return ad


@functools.lru_cache(maxsize=None)
def planted_case():
    """The planted case of seed 0 with its three oracle results: the top-5 % profile, the clone means, both by the
    contract of tl.cnv_pseudobulk."""
    c = co.planted(0)
    rows, top_profile = co.top_profile(c["x"], 0.05)
    means = pb.profiles(c["x"], c["clone"], 3)["mean"]
    return c, rows, co.correlate(c["x"], top_profile), means, co.correlate(c["x"], means)


def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _assert_written(ad, want, names, key="cnv_correlation"):
    assert co.same_bytes(_host(ad.obsm[f"X_{key}"]), want["r"])
    assert ad.obs[key].dtype == np.float64 and co.same_bytes(ad.obs[key].to_numpy(), want["best_r"])
    column = ad.obs[f"{key}_profile"]
    assert isinstance(column.dtype, pd.CategoricalDtype) and list(column.cat.categories) == names
    assert np.array_equal(column.cat.codes.to_numpy(), want["best_g"])


def test_the_top_mode_separates_the_planted_tumour_cells():
    import infercnvpy_amd as cnv

    c, rows, want, _, _ = planted_case()
    tumour = c["clone"] >= 0
    ad = _adata(c["x"])
    r, names, info = cnv.tl.cnv_correlation(ad, return_info=True)
    assert isinstance(r, np.ndarray) and r is ad.obsm["X_cnv_correlation"] and names == ["top"]
    _assert_written(ad, want, ["top"])
    uns = ad.uns["cnv_correlation"]
    assert set(uns) == {"profiles", "source", "use_rep", "groupby", "top_fraction", "top_rows"}
    assert (uns["profiles"], uns["source"], uns["use_rep"], uns["groupby"], uns["top_fraction"]) == (
        ["top"], "top", "cnv", None, 0.05)
    assert uns["top_rows"].dtype == np.int64 and np.array_equal(uns["top_rows"], rows)
    assert info["n_profiles"] == 1 and info["source"] == "top" and set(info["stage_ms"]) == {"profiles", "correlation"}
    outside = np.ones(240, dtype=bool)
    outside[rows] = False
    assert r[tumour & outside, 0].min() > r[~tumour, 0].max()
    # the signal: B / W of the same pass, byte for byte
    cnv.tl.cnv_signal(ad)
    assert ad.obs["cnv_signal"].dtype == np.float64 and co.same_bytes(ad.obs["cnv_signal"].to_numpy(), want["signal"])
    assert co.same_bytes(want["signal"], want["B"] / 270.0)
    assert ad.obs["cnv_signal"].to_numpy()[~tumour].max() > ad.obs["cnv_signal"].to_numpy()[tumour].min()
    # another fraction, another key, the sparse form of the matrix
    ad = _adata(sp.csr_matrix(c["x"]))
    cnv.tl.cnv_correlation(ad, top_fraction="1/4", key_added="other")
    rows4, profile4 = co.top_profile(c["x"], "1/4")
    assert rows4.shape == (60,) and np.array_equal(ad.uns["other"]["top_rows"], rows4)
    _assert_written(ad, co.correlate(c["x"], profile4), ["top"], key="other")
    assert ad.uns["other"]["top_fraction"] == 0.25


def test_groupby_and_profiles_assign_every_tumour_cell_to_its_clone():
    import torch

    import infercnvpy_amd as cnv

    c, _, _, means, want = planted_case()
    tumour = c["clone"] >= 0
    names = ["clone0", "clone1", "clone2"]
    ad = _adata(c["x"], c["clone"])
    cnv.tl.cnv_correlation(ad, groupby="clone")
    _assert_written(ad, want, names)
    assert ad.uns["cnv_correlation"] == {"profiles": names, "source": "groupby", "use_rep": "cnv", "groupby": "clone",
                                         "top_fraction": None}
    assert np.array_equal(ad.obs["cnv_correlation_profile"].cat.codes.to_numpy()[tumour], c["clone"][tumour])
    assert ad.obs["cnv_correlation_profile"].tolist()[:3] == [names[g] for g in want["best_g"][:3]]
    # the container of tl.cnv_pseudobulk, on the cells of "another sample" (here: the rows in reverse order)
    clones = cnv.tl.cnv_pseudobulk(ad, "clone")
    assert clones.X.tobytes() == means.tobytes()
    other = _adata(np.ascontiguousarray(c["x"][::-1]))
    cnv.tl.cnv_correlation(other, clones)
    _assert_written(other, {k: v[::-1] for k, v in want.items()}, names)
    assert other.uns["cnv_correlation"]["source"] == "profiles" and other.uns["cnv_correlation"]["groupby"] is None
    # an array and a CUDA tensor of profiles: named by their number
    for given in (means, means.tolist(), torch.from_numpy(means).cuda()):
        r, numbered = cnv.tl.cnv_correlation(_adata(c["x"]), given, inplace=False)
        assert numbered == ["0", "1", "2"] and co.same_bytes(r, want["r"])
    # a row that is NaN against every profile has no best profile
    x = c["x"].copy()
    x[4] = 0.0
    ad = _adata(x)
    cnv.tl.cnv_correlation(ad, means)
    assert np.isnan(ad.obs["cnv_correlation"].iloc[4]) and pd.isna(ad.obs["cnv_correlation_profile"].iloc[4])
    assert ad.obs["cnv_correlation_profile"].cat.codes.iloc[4] == -1


def test_device_input_stays_on_the_device_and_inplace_false_writes_nothing():
    import torch

    import infercnvpy_amd as cnv

    c, rows, want_top, means, want = planted_case()
    for x in (torch.from_numpy(c["x"]).cuda(), _inputs(sp.csr_matrix(c["x"]))["packed_csr_with_a_tail"]):
        ad = _adata(x, c["clone"])
        out = cnv.tl.cnv_correlation(ad, groupby="clone", inplace=False)
        assert set(ad.obsm) == {"X_cnv"} and list(ad.obs.columns) == ["clone"] and set(ad.uns) == {"cnv"}
        r, names = out
        assert torch.is_tensor(r) and r.is_cuda and r.dtype == torch.float64 and names == ["clone0", "clone1", "clone2"]
        assert co.same_bytes(r.cpu().numpy(), want["r"])
        assert cnv.tl.cnv_correlation(ad, key_added="top") is None
        assert torch.is_tensor(ad.obsm["X_top"]) and ad.obsm["X_top"].is_cuda
        _assert_written(ad, want_top, ["top"], key="top")
        assert np.array_equal(ad.uns["top"]["top_rows"], rows)
        signal = cnv.tl.cnv_signal(ad, inplace=False)
        assert isinstance(signal, np.ndarray) and co.same_bytes(signal, want["signal"]) and "cnv_signal" not in ad.obs.columns


def test_non_finite_values_are_refused():
    import infercnvpy_amd as cnv

    c = planted_case()[0]
    tumour_row, normal_row = int(np.flatnonzero(c["clone"] >= 0)[0]), int(np.flatnonzero(c["clone"] < 0)[0])
    for bad in (np.nan, np.inf):
        x = sp.csr_matrix(c["x"])
        x.data[normal_row * 270 + 7] = bad  # (a cell of no group: tl.cnv_pseudobulk meets it in its magnitude check)
        with pytest.raises(ValueError, match="tl.cnv_pseudobulk: X_cnv has a stored value of magnitude"):
            cnv.tl.cnv_correlation(_adata(x, c["clone"]), groupby="clone")
        x = sp.csr_matrix(c["x"])
        x.data[tumour_row * 270 + 7] = bad
        for kw in ({}, {"groupby": "clone"}, {"profiles": np.ones((1, 270)) * np.arange(270)}):
            ad = _adata(x, c["clone"])
            with pytest.raises(ValueError, match="X_cnv has non-finite values"):
                cnv.tl.cnv_correlation(ad, **kw)
            assert set(ad.obsm) == {"X_cnv"} and list(ad.obs.columns) == ["clone"]
        with pytest.raises(ValueError, match="tl.cnv_signal: X_cnv has non-finite values"):
            cnv.tl.cnv_signal(_adata(x))


def test_a_real_anndata_with_host_csr_input():
    anndata = pytest.importorskip("anndata")
    import infercnvpy_amd as cnv

    c, rows, want_top, _, want = planted_case()
    obs = pd.DataFrame({"clone": pd.Categorical.from_codes(c["clone"], categories=["clone0", "clone1", "clone2"])},
                       index=[f"cell{i}" for i in range(240)])
    ad = anndata.AnnData(X=sp.csr_matrix(np.zeros((240, 2), dtype=np.float32)), obs=obs)
    ad.obsm["X_cnv"] = sp.csr_matrix(c["x"])
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 140}}
    cnv.tl.cnv_correlation(ad)
    cnv.tl.cnv_correlation(ad, groupby="clone", key_added="by_clone")
    cnv.tl.cnv_signal(ad)
    _assert_written(ad, want_top, ["top"])
    _assert_written(ad, want, ["clone0", "clone1", "clone2"], key="by_clone")
    assert np.array_equal(ad.uns["cnv_correlation"]["top_rows"], rows)
    assert co.same_bytes(ad.obs["cnv_signal"].to_numpy(), want["signal"])

"""tl.cnv_copy_states_fit on the GPU equals the oracle of DESIGN.md 4.24 (tests/_copy_fit_oracle.py): the E-step's
statistics on the float64 bytes for every chromosome layout, every K, the kernel's own chr_start array and the LDS bound,
the stay mass against the three-state kernel, the whole trajectory of the fit, every kind of input, the chain into
tl.cnv_copy_states and tl.cnv_copy_posteriors on the planted case, and the edge cases."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import _copy_fit_oracle as cfo
import _copy_posterior_oracle as cpo
import _copy_states_oracle as co
import _fit_oracle as fo
import _states_oracle as so

pytestmark = pytest.mark.gpu

SEED = 2  # the planted case of the trajectory and chain tests
SIX = dict(levels=cfo.levels_of(co.DEFAULT_STEPS, 0.3), sigma=0.1, switch_prob=1e-3)  # the K = 6 default levels


def _adata(x, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _fit(x, chr_pos, **kw):
    import infercnvpy_amd as cnv

    return cnv.tl.cnv_copy_states_fit(_adata(x, chr_pos), inplace=False, return_info=True, **kw)


def _stats(x, bounds, levels, sigma, switch_prob):
    """The kernel's statistics as a host array; bounds: the chr_start array."""
    from infercnvpy_amd import _engine

    mu, z = co.check_levels(levels)
    h, ps, pw = cpo.scalars(sigma, switch_prob, len(mu))
    dm = _engine.matrix_input(x, "test")
    got = _engine.copy_posterior_stats(dm, np.asarray(bounds, dtype=np.int32), levels=mu, neutral=z, h=h, ps=ps, pw=pw)
    assert got.is_cuda and str(got.dtype) == "torch.float64" and tuple(got.shape) == (x.shape[0], 2 * len(mu) + 1)
    return got.cpu().numpy()


def _check_stats(name, x, chr_pos, levels, sigma, switch_prob, bounds=None):
    want = cfo.stats(x, chr_pos, levels, sigma, switch_prob, bounds=bounds)
    assert np.isfinite(want).all()
    edges = so.bounds(chr_pos, x.shape[1]) if bounds is None else bounds
    got = _stats(x, edges, levels, sigma, switch_prob)
    differ = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    worst = float(np.nanmax(np.abs(got - want))) if differ else 0.0
    print(f"{name}: {want.shape}, {differ} values differ from the oracle, largest difference {worst:.3g}")
    assert got.tobytes() == want.tobytes(), name
    return got


@functools.lru_cache(maxsize=None)
def _planted(fit):
    """The planted matrix of the trajectory tests and the oracle's fit of it, computed once."""
    c = co.planted_levels(SEED)
    return c, cfo.cnv_copy_states_fit(c["x"], c["chr_pos"], fit=fit)


def _same_fit(params, info, want, what):
    """params, history, n_iter, converged, fit, amplitude and steps against the oracle's, as reprs (a float's repr is its
    bits)."""
    assert repr(params) == repr(want["params"]), what
    assert repr(info["history"]) == repr(want["history"]), what
    assert (info["n_iter"], info["converged"], info["fit"]) == (want["n_iter"], want["converged"], want["fit"]), what
    assert repr((info["amplitude"], info["steps"])) == repr((want["amplitude"], want["steps"])), what
    assert info.get("stopped") == want.get("stopped"), what
    assert set(info["stage_ms"]) == {"rowsq", "e_steps"}, what


# ---- the statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cpo.SHAPE_NAMES)
def test_statistics_of_every_chromosome_layout_equal_the_oracle(name):
    """K = 6 default levels; one_window_chromosome_between_long needs the LDS tail (2K + 1 sums, K + 1 plane slots),
    chromosomes_65 and chromosomes_130 have more chromosomes than lanes."""
    c = co.shapes()[name]
    _check_stats(name, so.canonical(c["x"]), c["chr_pos"], **SIX)


@pytest.mark.parametrize("p", co.EVERY_K_SWITCH)
@pytest.mark.parametrize("k, z", [(2, 0), (2, 1), (3, 1), (5, 2), (5, 4), (8, 3), (8, 0)])
def test_statistics_of_every_k_equal_the_oracle(k, z, p):
    c = co.every_k(k, z, p)
    kw = c["kwargs"]
    _check_stats(f"every_k_{k}_{z}_{p}", c["x"], c["chr_pos"], kw["levels"], kw["sigma"], kw["switch_prob"])


def test_statistics_under_the_kernels_own_chr_start_array():
    """An empty chromosome and windows that no chromosome covers add nothing."""
    c = so.planted(6, [10, 7, 13], 19)
    whole = _check_stats("whole", c["x"], c["chr_pos"], **SIX)
    empty = _check_stats("empty chromosome", c["x"], c["chr_pos"], bounds=[0, 10, 10, 17, 30], **SIX)
    assert empty.tobytes() == whole.tobytes()
    part = _check_stats("uncovered windows", c["x"], c["chr_pos"], bounds=[3, 9, 28], **SIX)
    alone = cfo.stats(c["x"][:, 3:28], {"a": 0, "b": 6}, **SIX)
    assert part.tobytes() == alone.tobytes() and part.tobytes() != whole.tobytes()


def test_statistics_at_the_lds_bound_and_the_refusal_above_it(monkeypatch):
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib

    w = (163840 - 8 * 13) // 56
    assert w == 2923 == cfo.max_windows(6, 1) and cfo.lds_bytes(w, 6, 1) <= cfo.LDS_BYTES < cfo.lds_bytes(w + 1, 6, 1)
    c = so.planted(2, [w], 66)
    assert c["x"].shape == (2, w) and len(c["chr_pos"]) == 1
    _check_stats("lds bound", c["x"], c["chr_pos"], **SIX)
    wide = so.planted(2, [w + 1], 66)["x"]
    with pytest.raises(ValueError, match="163840"):
        _stats(wide, [0, w + 1], **SIX)
    assert str(w) in _lib.load().icv_last_error().decode()

    def launched(*a, **kw):
        raise AssertionError("the kernel was launched above its LDS bound")

    monkeypatch.setattr(_engine, "copy_posterior_stats", launched)
    with pytest.raises(ValueError, match=f"163840.*at most {w}"):
        cnv.tl.cnv_copy_states_fit(_adata(wide, {"chr1": 0}), amplitude=0.3, sigma=0.1)


@pytest.mark.parametrize("name", ["planted", "one_window_chromosome_between_long", "chromosomes_130"])
def test_stay_mass_is_the_bytes_of_the_three_state_kernel(name):
    from infercnvpy_amd import _engine
    from infercnvpy_amd.tl._hmm import chromosome_bounds

    c = co.planted_levels(SEED) if name == "planted" else co.shapes()[name]
    x = so.canonical(c["x"])
    bounds = chromosome_bounds(c["chr_pos"], x.shape[1])
    for a, sigma, p in ((0.3, 0.1, 1e-3), (0.23, 0.17, 0.3)):
        got = _stats(x, bounds, (-a, 0.0, a), sigma, p)
        h, ps, pw = cpo.scalars(sigma, p, 3)
        three = _engine.posterior_stats(_engine.matrix_input(x, "test"), bounds, amplitude=a, h=h, ps=ps, pw=pw).cpu().numpy()
        assert np.array_equal(got[:, 6], three[:, 2]) and got[:, 6].tobytes() == three[:, 2].tobytes(), (name, a)
        assert got[:, 6].tobytes() == fo.stats(x, c["chr_pos"], a, sigma, p)[:, 2].tobytes()


def _sums_of_the_planes(planes, x, bounds):
    """N_s and M_s of DESIGN.md 4.24 from the posteriors gamma (K x n x W): per chromosome from t = T - 1 down to 0, the
    product gamma x rounded before the add, then the chromosomes in ascending order from 0.0.  Python floats: every
    operation is one float64 operation."""
    k, n, _ = planes.shape
    out = np.zeros((n, 2 * k), dtype=np.float64)
    for i in range(n):
        for s in range(k):
            n_acc, m_acc = 0.0, 0.0
            for s0, s1 in zip(bounds[:-1], bounds[1:]):
                n_chr, m_chr = 0.0, 0.0
                for t in range(int(s1) - 1, int(s0) - 1, -1):
                    ga = float(planes[s, i, t])
                    n_chr += ga
                    m_chr += ga * float(x[i, t])
                n_acc += n_chr
                m_acc += m_chr
            out[i, s], out[i, k + s] = n_acc, m_acc
    return out


@pytest.mark.parametrize("layout", ["chromosome_of_one_window", "seventy_chromosomes"])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_statistics_are_the_sums_of_the_planes_the_chains_kernel_writes(k, layout):
    """icv_copy_posterior_stats and icv_copy_posterior_chains run one chain, each in its own body: N_s and M_s are the
    sums of the planes the chains kernel writes, bit for bit.  [0, 1, 4, 9]: a chromosome of one window has no inner
    window and no window t - 1 to read; 70 chromosomes of one or two windows: lanes take a second chromosome.  S stays
    with the oracle tests above."""
    from infercnvpy_amd import _engine

    if layout == "chromosome_of_one_window":
        bounds = np.array([0, 1, 4, 9], dtype=np.int32)
    else:
        bounds = np.concatenate([[0], np.cumsum([1 + c % 2 for c in range(70)])]).astype(np.int32)
    n, w = 5, int(bounds[-1])
    rng = np.random.default_rng(100 * k + w)
    dense32 = (rng.normal(0.0, 0.3, (n, w)) * (rng.random((n, w)) < 0.6)).astype(np.float32)
    dense32[3] = 0.0  # a row without a stored entry
    z = k // 2
    mu = [(s - z) * 0.3 for s in range(k)]
    h, ps, pw = cpo.scalars(0.2, 0.01, k)
    for name, x in (("dense_float32", dense32), ("dense_float64", dense32.astype(np.float64)),
                    ("csr_float32", sp.csr_matrix(dense32)), ("csr_float64", sp.csr_matrix(dense32.astype(np.float64)))):
        dm = _engine.matrix_input(x, "test")
        _, planes = _engine.copy_posterior_chains(dm, bounds, levels=mu, neutral=z, h=h, ps=ps, pw=pw, all_states=True)
        stats = _engine.copy_posterior_stats(dm, bounds, levels=mu, neutral=z, h=h, ps=ps, pw=pw).cpu().numpy()
        want = _sums_of_the_planes(planes.cpu().numpy(), dense32.astype(np.float64), bounds)
        assert np.isfinite(want).all() and stats.shape == (n, 2 * k + 1), name
        differ = int((stats[:, :2 * k].view(np.uint64) != want.view(np.uint64)).sum())
        print(f"{layout}, K = {k}, {name}: {differ} of {want.size} sums differ from the sums of the planes")
        assert np.ascontiguousarray(stats[:, :2 * k]).tobytes() == want.tobytes(), name
        assert np.array_equal(stats[3, k:2 * k], np.zeros(k)) and stats[3, :k].sum() == pytest.approx(w), name


def test_every_kind_of_input_gives_the_same_bytes():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(150, [66, 1, 140, 14], 21)
    dense32 = c["x"].toarray().astype(np.float32)  # float32 numbers: exactly representable in every form below
    x = sp.csr_matrix(dense32.astype(np.float64))
    pos = c["chr_pos"]
    edges = so.bounds(pos, x.shape[1])
    want_stats = cfo.stats(x, pos, **SIX)
    want = cfo.cnv_copy_states_fit(x, pos)
    dev_csr = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                            torch.from_numpy(x.indices.astype(np.int32)).cuda(), torch.from_numpy(x.data).cuda(),
                            x.shape[1])
    inputs = {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
              "dense_float64": dense32.astype(np.float64), "packed_csr": dev_csr,
              "cuda_float32": torch.from_numpy(dense32).cuda(), "cuda_float64": torch.from_numpy(dense32).cuda().double()}
    plane = x.shape[0] * x.shape[1]  # the bytes of the smallest n x W tensor there could be (int8)
    for name, xin in inputs.items():
        assert _stats(xin, edges, **SIX).tobytes() == want_stats.tobytes(), name
        on_device = name in ("packed_csr", "cuda_float32", "cuda_float64")
        if on_device:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
        params, info = _fit(xin, pos)
        if on_device:  # neither left behind nor allocated on the way
            assert torch.cuda.memory_allocated() - before < plane, name
            assert torch.cuda.max_memory_allocated() - before < plane, name
        _same_fit(params, info, want, name)
        assert all(type(v) is float for v in params["levels"]) and type(params["sigma"]) is float, name
    assert want["converged"] and want["n_iter"] >= 3


# ---- the fit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [("amplitude", "sigma"), cfo.NAMES], ids=["default", "all_three"])
def test_whole_trajectory_equals_the_oracle(fit):
    c, want = _planted(fit)
    params, info = _fit(c["x"], c["chr_pos"], **({} if fit == ("amplitude", "sigma") else {"fit": fit}))
    print(f"{info['n_iter']} iterations, converged {info['converged']}: {params}")
    _same_fit(params, info, want, str(fit))
    assert want["n_iter"] >= 3 and want["converged"] and info["fit"] == list(fit)


def test_fitted_parameters_drive_cnv_copy_states_and_cnv_copy_posteriors():
    import infercnvpy_amd as cnv

    c, want = _planted(("amplitude", "sigma"))
    ad = _adata(c["x"], c["chr_pos"])
    assert cnv.tl.cnv_copy_states_fit(ad) is None
    stored = ad.uns["cnv_copy_states_fit"]
    keys = ("params", "amplitude", "steps", "history", "n_iter", "converged", "fit")
    assert set(stored) == set(keys) and set(stored["params"]) == {"levels", "sigma", "switch_prob"}
    assert repr(stored) == repr({k: want[k] for k in keys})
    fitted = stored["params"]
    cnv.tl.cnv_copy_states(ad, **fitted)
    cnv.tl.cnv_copy_posteriors(ad)
    states, sign, fraction, params = co.cnv_copy_states(c["x"], c["chr_pos"], **want["params"])
    assert ad.obsm["X_cnv_copy_states"].tobytes() == states.tobytes()
    assert ad.obsm["X_cnv_copy_states_sign"].tobytes() == sign.tobytes()
    assert np.asarray(ad.obs["cnv_copy_states_fraction"]).tobytes() == fraction.tobytes()
    assert repr(ad.uns["cnv_copy_states"]["params"]) == repr(params) == repr(ad.uns["cnv_copy_posterior"]["params"])
    assert repr({k: params[k] for k in fitted}) == repr(fitted) and params["neutral"] == 2
    planes, _ = cpo.cnv_copy_posteriors(c["x"], c["chr_pos"], **want["params"])
    assert ad.obsm["X_cnv_copy_posterior_neutral"].tobytes() == planes[2].tobytes()
    wrong = int((ad.obsm["X_cnv_copy_states"] != c["truth"]).sum())
    default = int((co.cnv_copy_states(c["x"], c["chr_pos"])[0] != c["truth"]).sum())
    print(f"{wrong} wrong calls with the fitted parameters, {default} with the defaults")
    assert wrong == cfo.PLANTED_WRONG[SEED] <= co.PLANTED_MOST_WRONG < 500 <= default


def test_inplace_false_return_info_second_call_and_max_iter():
    import infercnvpy_amd as cnv

    c, want = _planted(("amplitude", "sigma"))
    ad = _adata(c["x"], c["chr_pos"])
    params = cnv.tl.cnv_copy_states_fit(ad, inplace=False)
    assert repr(params) == repr(want["params"]) and "cnv_copy_states_fit" not in ad.uns
    none, info = cnv.tl.cnv_copy_states_fit(ad, return_info=True)
    assert none is None and info["n_iter"] == want["n_iter"] and "stopped" not in info
    first = repr(ad.uns["cnv_copy_states_fit"])
    cnv.tl.cnv_copy_states_fit(ad, key_added="again")  # a second call on the same adata
    assert repr(ad.uns["again"]) == first and repr(ad.uns["cnv_copy_states_fit"]) == first
    # max_iter ends the loop before convergence; the history is a prefix
    params, info = _fit(c["x"], c["chr_pos"], max_iter=2)
    assert info["n_iter"] == 2 and not info["converged"] and repr(info["history"]) == repr(want["history"][:3])
    assert repr(params["levels"]) == repr(cfo.levels_of(co.DEFAULT_STEPS, want["history"][2]["amplitude"]))


def test_steps_subsets_start_values_and_one_window():
    c = co.planted_levels(SEED)
    for kw in ({"steps": (-1, 0, 1, 2, 3)}, {"steps": (0, 1, 2, 3), "fit": ("sigma",), "amplitude": 0.31, "switch_prob": 0.01},
               {"fit": ("switch_prob",), "sigma": 0.1, "amplitude": 0.3}, {"steps": [-1, 0, 1], "tol": 0.0, "max_iter": 3},
               {"sigma": 0.33, "max_iter": 4}):
        params, info = _fit(c["x"], c["chr_pos"], **kw)
        _same_fit(params, info, cfo.cnv_copy_states_fit(c["x"], c["chr_pos"], **kw), str(kw))
    one = co.shapes()["one_window"]  # no chromosome has two windows: the root mean square starts the fit
    kw = {"fit": cfo.NAMES, "switch_prob": 0.02}
    params, info = _fit(one["x"], one["chr_pos"], **kw)
    _same_fit(params, info, cfo.cnv_copy_states_fit(one["x"], one["chr_pos"], **kw), "one_window")
    assert params["switch_prob"] == 0.02 and info["n_iter"] >= 1
    assert info["history"][0]["sigma"] == so.default_sigma(so.canonical(one["x"]))


def test_all_zero_matrix_returns_zero_levels_without_an_iteration():
    import torch

    pos = {"chr1": 0, "chr2": 17}
    for x in (sp.csr_matrix((5, 40)), np.zeros((5, 40), dtype=np.float32), torch.zeros((5, 40), device="cuda")):
        params, info = _fit(x, pos)
        assert params == {"levels": [0.0] * 6, "sigma": 0.0, "switch_prob": 1e-3}
        assert info["n_iter"] == 0 and not info["converged"] and info["amplitude"] == 0.0
        assert info["history"] == [{"amplitude": 0.0, "sigma": 0.0, "switch_prob": 1e-3}]
        _same_fit(params, info, cfo.cnv_copy_states_fit(sp.csr_matrix((5, 40)), pos), "all zero")


def test_degenerate_step_warns_and_keeps_the_previous_parameters():
    x, pos, kw = fo.degenerate_case()
    want = cfo.cnv_copy_states_fit(x, pos, **kw)
    assert want["stopped"] == "degenerate"
    with pytest.warns(RuntimeWarning, match="variance"):
        params, info = _fit(x, pos, **kw)
    _same_fit(params, info, want, "degenerate")
    assert params == {"levels": cfo.levels_of(co.DEFAULT_STEPS, 0.5), "sigma": 1e-3, "switch_prob": 1e-3}
    assert info["n_iter"] == 1 and info["stopped"] == "degenerate"
    with warnings.catch_warnings(record=True) as seen:  # nothing divides by the variance: no warning
        warnings.simplefilter("always")
        params, info = _fit(x, pos, fit=("amplitude",), **kw)
    assert not [w for w in seen if "cnv_copy_states_fit" in str(w.message)]
    _same_fit(params, info, cfo.cnv_copy_states_fit(x, pos, fit=("amplitude",), **kw), "amplitude alone")


def test_nonfinite_values_raise():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(40, [20, 9], 5)
    for bad in (np.nan, np.inf):
        x = c["x"].copy()
        x.data[x.indptr[17]] = bad
        for xin in (x, torch.from_numpy(x.toarray()).cuda()):
            for kw in ({}, {"sigma": 0.2, "amplitude": 0.4}):
                ad = _adata(xin, c["chr_pos"])
                with pytest.raises(ValueError, match="non-finite"):
                    cnv.tl.cnv_copy_states_fit(ad, **kw)
                assert "cnv_copy_states_fit" not in ad.uns

"""tl.cnv_states_fit on the GPU equals the oracle of DESIGN.md 4.16 (tests/_fit_oracle.py): the E-step's statistics on
the float64 bytes for every chromosome layout of the posterior cases, the whole trajectory of the fit, every kind of
input, the chain into tl.cnv_states and tl.cnv_posteriors, and the errors."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import _fit_oracle as fo
import _posterior_oracle as po
import _states_oracle as so

pytestmark = pytest.mark.gpu

SMALL = (60, [30, 7, 41, 1, 22], 5)


def _adata(x, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _fit(x, chr_pos, **kw):
    import infercnvpy_amd as cnv

    return cnv.tl.cnv_states_fit(_adata(x, chr_pos), inplace=False, return_info=True, **kw)


@functools.lru_cache(maxsize=None)
def _small(fit):
    """The planted matrix of the trajectory tests and the oracle's fit of it, computed once."""
    c = so.planted(*SMALL)
    return c, fo.cnv_states_fit(c["x"], c["chr_pos"], fit=fit)


def _same_fit(params, info, want, what):
    """params, history, n_iter, converged and fit against the oracle's, as reprs (a float's repr is its bits)."""
    assert repr(params) == repr(want["params"]), what
    assert repr(info["history"]) == repr(want["history"]), what
    assert (info["n_iter"], info["converged"], info["fit"]) == (want["n_iter"], want["converged"], want["fit"]), what
    assert info.get("stopped") == want.get("stopped"), what
    assert set(info["stage_ms"]) == {"rowsq", "e_steps"}, what


@pytest.mark.parametrize("name", po.CASE_NAMES)
def test_statistics_of_every_case_equal_the_oracle(name):
    from infercnvpy_amd import _engine
    from infercnvpy_amd.tl._states import chromosome_bounds

    c = po.case(name)
    p = c["params"]
    want = fo.stats(c["x"], c["chr_pos"], p["amplitude"], p["sigma"], p["switch_prob"])
    assert np.isfinite(want).all()
    h, ps, pw = po.scalars(p["sigma"], p["switch_prob"])
    dm = _engine.matrix_input(c["x"], "test")
    got = _engine.posterior_stats(dm, chromosome_bounds(c["chr_pos"], c["x"].shape[1]), amplitude=p["amplitude"], h=h,
                                  ps=ps, pw=pw)
    assert got.is_cuda and str(got.dtype) == "torch.float64" and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    differ = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    worst = float(np.nanmax(np.abs(got - want))) if differ else 0.0
    print(f"{name}: {want.shape}, {differ} values differ from the oracle, largest difference {worst:.3g}")
    assert got.tobytes() == want.tobytes(), name


@pytest.mark.parametrize("fit", [fo.NAMES, ("amplitude", "sigma")], ids=["all_three", "default"])
def test_whole_trajectory_equals_the_oracle(fit):
    c, want = _small(fit)
    params, info = _fit(c["x"], c["chr_pos"], fit=fit)
    print(f"{info['n_iter']} iterations, converged {info['converged']}: {params}")
    _same_fit(params, info, want, str(fit))
    assert want["n_iter"] >= 3 and want["converged"]


def test_default_fit_is_amplitude_and_sigma_and_inplace_stores_the_result():
    import infercnvpy_amd as cnv

    c, want = _small(("amplitude", "sigma"))
    ad = _adata(c["x"], c["chr_pos"])
    assert cnv.tl.cnv_states_fit(ad) is None
    stored = ad.uns["cnv_states_fit"]
    assert set(stored) == {"params", "history", "n_iter", "converged", "fit"}
    assert repr(stored) == repr({k: want[k] for k in ("params", "history", "n_iter", "converged", "fit")})
    none, info = cnv.tl.cnv_states_fit(ad, key_added="again", return_info=True)
    assert none is None and repr(ad.uns["again"]) == repr(stored) and info["n_iter"] == want["n_iter"]
    # max_iter ends the loop before convergence; the history is a prefix
    params, info = _fit(c["x"], c["chr_pos"], max_iter=2)
    assert info["n_iter"] == 2 and not info["converged"] and repr(info["history"]) == repr(want["history"][:3])
    assert repr(params) == repr(want["history"][2])


def test_every_kind_of_input_gives_the_same_parameters():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(150, [33, 1, 70, 7], 21)
    dense32 = c["x"].toarray().astype(np.float32)  # float32 numbers: exactly representable in every form below
    x = sp.csr_matrix(dense32.astype(np.float64))
    pos = c["chr_pos"]
    want = fo.cnv_states_fit(x, pos)
    dev_csr = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                            torch.from_numpy(x.indices.astype(np.int32)).cuda(), torch.from_numpy(x.data).cuda(),
                            x.shape[1])
    inputs = {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
              "dense_float64": dense32.astype(np.float64), "packed_csr": dev_csr,
              "cuda_float32": torch.from_numpy(dense32).cuda(), "cuda_float64": torch.from_numpy(dense32).cuda().double()}
    first = None
    plane = x.shape[0] * x.shape[1]  # the bytes of the smallest n x W tensor there could be (int8)
    for name, xin in inputs.items():
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
        first = first or (params, info["history"])
        assert repr((params, info["history"])) == repr(first), name
        assert all(isinstance(v, float) for v in params.values()), name
    assert want["converged"] and want["n_iter"] >= 3


def test_fitted_parameters_drive_cnv_states_and_cnv_posteriors():
    import infercnvpy_amd as cnv

    c, want = _small(("amplitude", "sigma"))
    ad = _adata(c["x"], c["chr_pos"])
    cnv.tl.cnv_states_fit(ad)
    fitted = ad.uns["cnv_states_fit"]["params"]
    cnv.tl.cnv_states(ad, **fitted)
    cnv.tl.cnv_posteriors(ad)
    states, fraction, params = so.cnv_states(c["x"], c["chr_pos"], **want["params"])
    assert ad.obsm["X_cnv_states"].tobytes() == states.tobytes()
    assert np.asarray(ad.obs["cnv_states_fraction"]).tobytes() == fraction.tobytes()
    assert repr(ad.uns["cnv_states"]["params"]) == repr(params) == repr(want["params"]) == repr(fitted)
    assert repr(ad.uns["cnv_posterior"]["params"]) == repr(fitted)
    neutral = po.cnv_posteriors(c["x"], c["chr_pos"], **want["params"])[1]
    assert ad.obsm["X_cnv_posterior_neutral"].tobytes() == neutral.tobytes()
    default = so.cnv_states(c["x"], c["chr_pos"])[0]
    wrong_default, wrong_fitted = int((default != c["truth"]).sum()), int((states != c["truth"]).sum())
    print(f"{wrong_fitted} wrong calls with the fitted parameters, {wrong_default} with the defaults")
    assert wrong_fitted < wrong_default


def test_subsets_start_values_one_window_and_second_call():
    c = so.planted(*SMALL)
    for kw in ({"fit": ("sigma",), "amplitude": 0.55, "switch_prob": 0.01}, {"fit": ("switch_prob",), "sigma": 0.08},
               {"fit": ["sigma", "amplitude"], "tol": 0.0, "max_iter": 3}):
        params, info = _fit(c["x"], c["chr_pos"], **kw)
        _same_fit(params, info, fo.cnv_states_fit(c["x"], c["chr_pos"], **kw), str(kw))
    one = po.case("one_window")
    kw = {"fit": fo.NAMES, "switch_prob": 0.02}
    params, info = _fit(one["x"], one["chr_pos"], **kw)
    _same_fit(params, info, fo.cnv_states_fit(one["x"], one["chr_pos"], **kw), "one_window")
    assert params["switch_prob"] == 0.02 and info["n_iter"] >= 1
    many = po.case("chromosomes_130")
    a, b = _fit(many["x"], many["chr_pos"], fit=fo.NAMES), _fit(many["x"], many["chr_pos"], fit=fo.NAMES)
    assert repr((a[0], a[1]["history"])) == repr((b[0], b[1]["history"]))
    _same_fit(*a, fo.cnv_states_fit(many["x"], many["chr_pos"], fit=fo.NAMES), "chromosomes_130")


def test_all_zero_matrix_returns_zeros_without_an_iteration():
    import torch

    pos = {"chr1": 0, "chr2": 17}
    for x in (sp.csr_matrix((5, 40)), np.zeros((5, 40), dtype=np.float32), torch.zeros((5, 40), device="cuda")):
        params, info = _fit(x, pos)
        assert params == {"amplitude": 0.0, "sigma": 0.0, "switch_prob": 1e-3}
        assert info["n_iter"] == 0 and info["history"] == [params] and not info["converged"]


def test_degenerate_step_warns_and_keeps_the_previous_parameters():
    x, pos, kw = fo.degenerate_case()
    want = fo.cnv_states_fit(x, pos, **kw)
    assert want["stopped"] == "degenerate"
    with pytest.warns(RuntimeWarning, match="variance"):
        params, info = _fit(x, pos, **kw)
    _same_fit(params, info, want, "degenerate")
    assert params == {"amplitude": 0.5, "sigma": 1e-3, "switch_prob": 1e-3} and info["n_iter"] == 1
    with warnings.catch_warnings(record=True) as seen:  # nothing divides by the variance: no warning
        warnings.simplefilter("always")
        params, info = _fit(x, pos, fit=("amplitude",), **kw)
    assert not [w for w in seen if "cnv_states_fit" in str(w.message)]
    _same_fit(params, info, fo.cnv_states_fit(x, pos, fit=("amplitude",), **kw), "amplitude alone")


def test_errors():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(40, [20, 9], 5)
    pos = c["chr_pos"]
    for kw, match in (({"fit": ("amplitude", "mean")}, "fit"), ({"fit": ()}, "fit"), ({"max_iter": 0}, "max_iter"),
                      ({"tol": float("nan")}, "tol")):
        with pytest.raises(ValueError, match=match):
            cnv.tl.cnv_states_fit(_adata(c["x"], pos), **kw)
    for bad in (np.nan, np.inf):
        x = c["x"].copy()
        x.data[x.indptr[17]] = bad
        for xin in (x, torch.from_numpy(x.toarray()).cuda()):
            for kw in ({}, {"sigma": 0.2, "amplitude": 0.4}):
                ad = _adata(xin, pos)
                with pytest.raises(ValueError, match="non-finite"):
                    cnv.tl.cnv_states_fit(ad, **kw)
                assert "cnv_states_fit" not in ad.uns
    with pytest.raises(ValueError, match=str(po.MAX_WINDOWS)):
        cnv.tl.cnv_states_fit(_adata(sp.csr_matrix((2, po.MAX_WINDOWS + 1)), {"chr1": 0}))
    ad = _adata(c["x"], pos)
    with pytest.raises(KeyError, match="X_other not found in adata.obsm. Did you run `tl.infercnv`"):
        cnv.tl.cnv_states_fit(ad, use_rep="other")
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match=r"chr_pos not found in adata.uns\['cnv'\]. Did you run `tl.infercnv`"):
        cnv.tl.cnv_states_fit(ad)


@pytest.mark.parametrize("sigma", [None, 0.2], ids=["all_none", "sigma_given"])
def test_the_three_functions_resolve_one_model_from_one_matrix(sigma):
    """Why tl/_hmm.py exists: tl.cnv_states, tl.cnv_posteriors (on an adata without stored calls) and the start of
    tl.cnv_states_fit derive the same (amplitude, sigma, switch_prob), the oracle's, bit for bit."""
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(40, [20, 9], 5)
    pos = c["chr_pos"]
    dense32 = c["x"].toarray().astype(np.float32)
    for name, xin, host in (("csr_float64", c["x"], c["x"]), ("cuda_float32", torch.from_numpy(dense32).cuda(), dense32)):
        sig = so.default_sigma(host) if sigma is None else sigma
        want = {"amplitude": 2.0 * sig, "sigma": sig, "switch_prob": 1e-3}
        called, fresh = _adata(xin, pos), _adata(xin, pos)
        cnv.tl.cnv_states(called, sigma=sigma)
        cnv.tl.cnv_posteriors(fresh, sigma=sigma)
        assert "cnv_states" not in fresh.uns
        _, info = _fit(xin, pos, sigma=sigma, max_iter=1)
        models = [called.uns["cnv_states"]["params"], fresh.uns["cnv_posterior"]["params"], info["history"][0], want]
        assert all(type(m[k]) is float for m in models for k in fo.NAMES), name
        bits = [np.array([m[k] for k in fo.NAMES], dtype=np.float64).tobytes() for m in models]
        print(f"{name}: {models[0]}")
        assert bits[0] == bits[1] == bits[2] == bits[3], (name, models)

"""tl.cnv_copy_posteriors and tl.cnv_copy_states_filter on the GPU equal the oracle of DESIGN.md 4.23
(tests/_copy_posterior_oracle.py) byte for byte, and with three levels the bytes of tl.cnv_posteriors and of
icv_states_filter: every K and neutral position, every chromosome layout, the window cap of every K, every kind of
input, the stored parameters, the errors that need the device, the filter at its step boundaries on levels, and the
chain from the calls to the segment table on the planted multi-level case."""
import numpy as np
import pytest
import scipy.sparse as sp

import _copy_posterior_oracle as cpo
import _copy_states_oracle as co
import _posterior_oracle as po
import _segments_oracle as sg
import _states_oracle as so

pytestmark = pytest.mark.gpu
ALL_K = range(cpo.MIN_STATES, cpo.MAX_STATES + 1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _adata(x, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _run(x, chr_pos, **kw):
    import infercnvpy_amd as cnv

    return cnv.tl.cnv_copy_posteriors(_adata(x, chr_pos), inplace=False, **kw)


def _check_case(name):
    """All planes equal the oracle's bits, and the neutral-only call gives the neutral plane."""
    c = cpo.case(name)
    planes = _run(c["x"], c["chr_pos"], all_states=True, **c["kwargs"])
    k, z = c["planes"].shape[0], c["params"]["neutral"]
    assert isinstance(planes, tuple) and len(planes) == k
    differ = 0
    for got, want in zip(planes, c["planes"]):
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == c["x"].shape
        differ += int((_bits(got) != _bits(want)).sum())
    print(f"{name}: {c['planes'].shape}, {differ} float64 differ from the oracle")
    assert differ == 0
    neutral = _run(c["x"], c["chr_pos"], **c["kwargs"])
    assert isinstance(neutral, np.ndarray) and np.array_equal(_bits(neutral), _bits(planes[z]))
    return c


# ---- posteriors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exp_cutoff", "outliers", "chromosomes_130", "full_and_empty", "switch_0.3",
                                  "switch_1e-12", "switch_1e-3"])
def test_three_levels_give_the_bytes_of_cnv_posteriors(name):
    import infercnvpy_amd as cnv

    c = po.case(name)
    a, sigma, p = c["params"]["amplitude"], c["params"]["sigma"], c["params"]["switch_prob"]
    three = cnv.tl.cnv_posteriors(_adata(c["x"], c["chr_pos"]), inplace=False, amplitude=a, sigma=sigma, switch_prob=p,
                                  all_states=True)
    planes = _run(c["x"], c["chr_pos"], levels=(-a, 0.0, a), sigma=sigma, switch_prob=p, all_states=True)
    for got, ref, key in zip(planes, three, ("loss", "neutral", "gain")):
        print(f"{name} {key}: {int((_bits(got) != _bits(ref)).sum())} float64 differ from tl.cnv_posteriors, "
              f"{int((_bits(got) != _bits(c[key])).sum())} from the three-state oracle")
        assert got.tobytes() == ref.tobytes() == c[key].tobytes()


@pytest.mark.parametrize("k", ALL_K)
def test_every_k_and_neutral_position_equals_the_oracle(k):
    for z in range(k):
        for p in co.EVERY_K_SWITCH:
            c = _check_case(f"every_k_{k}_{z}_{p}")
            assert 30 <= c["x"].shape[0] <= 45 and c["params"]["neutral"] == z


@pytest.mark.parametrize("name", cpo.SHAPE_NAMES)
def test_every_chromosome_layout_equals_the_oracle(name):
    _check_case(name)


@pytest.mark.parametrize("k", ALL_K)
def test_the_window_cap_of_every_k(k, monkeypatch):
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    c = _check_case(f"cap_{k}")
    cap = cpo.max_windows(k)
    assert c["x"].shape == (2, cap) and len(c["chr_pos"]) == 1 and c["planes"].shape[0] == k

    def launched(*a, **kw):
        raise AssertionError("the kernel was launched above its window cap")

    monkeypatch.setattr(_engine, "copy_posterior_chains", launched)
    ad = _adata(sp.csr_matrix((2, cap + 1)), {"chr1": 0})
    with pytest.raises(ValueError, match=f"K = {k} states in LDS and takes at most {cap}"):
        cnv.tl.cnv_copy_posteriors(ad, **c["kwargs"])


def test_every_kind_of_input_gives_the_same_bytes():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(150, [33, 1, 70, 7], 21)
    dense32 = c["x"].toarray().astype(np.float32)  # float32 numbers: exactly representable in every form below
    x = sp.csr_matrix(dense32.astype(np.float64))
    pos = c["chr_pos"]
    kw = {"amplitude": 0.3, "sigma": 0.1}
    want, params = cpo.cnv_copy_posteriors(x, pos, **kw)
    dev_csr = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                            torch.from_numpy(x.indices.astype(np.int32)).cuda(), torch.from_numpy(x.data).cuda(),
                            x.shape[1])
    inputs = {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
              "dense_float64": dense32.astype(np.float64), "packed_csr": dev_csr,
              "cuda_float32": torch.from_numpy(dense32).cuda(), "cuda_float64": torch.from_numpy(dense32).cuda().double()}
    for name, xin in inputs.items():
        planes, info = _run(xin, pos, all_states=True, return_info=True, **kw)
        on_device = name in ("packed_csr", "cuda_float32", "cuda_float64")
        assert len(planes) == 6 and all(torch.is_tensor(v) == on_device for v in planes), name
        if on_device:
            assert all(v.is_cuda and v.dtype == torch.float64 for v in planes)
            planes = [v.cpu().numpy() for v in planes]
        assert info["levels"] == params["levels"] and info["neutral"] == 2 and info["sigma"] == 0.1, name
        assert info["switch_prob"] == 1e-3 and info["n_chromosomes"] == 4 and set(info["stage_ms"]) == {"rowsq", "chains"}
        for got, ref in zip(planes, want):
            assert np.array_equal(_bits(got), _bits(ref)), name
        neutral = _run(xin, pos, **kw)
        assert torch.is_tensor(neutral) == on_device
        assert np.array_equal(_bits(neutral.cpu().numpy() if on_device else neutral), _bits(want[2])), name


def test_parameters_are_picked_up_from_the_calls_and_results_are_stored():
    import torch

    import infercnvpy_amd as cnv

    c = cpo.case("one_window_chromosome_between_long")
    x, pos = c["x"], c["chr_pos"]
    kw = {"levels": (-0.25, 0.0, 0.3, 0.55, 0.9), "sigma": 0.12, "switch_prob": 0.01}
    want, params = cpo.cnv_copy_posteriors(x, pos, **kw)
    ad = _adata(x, pos)
    cnv.tl.cnv_copy_states(ad, **kw)
    assert ad.uns["cnv_copy_states"]["params"] == params
    assert cnv.tl.cnv_copy_posteriors(ad, all_states=True) is None
    names = ["loss1", "neutral", "gain1", "gain2", "gain3"]
    assert ad.uns["cnv_copy_posterior"] == {"params": params, "planes": names}
    for name, ref in zip(names, want):
        got = ad.obsm[f"X_cnv_copy_posterior_{name}"]
        assert isinstance(got, np.ndarray) and np.array_equal(_bits(got), _bits(ref)), name
    # an argument of the model switches the stored parameters off: the defaults of tl.cnv_copy_states apply
    default, default_params = cpo.cnv_copy_posteriors(x, pos, switch_prob=1e-3)
    cnv.tl.cnv_copy_posteriors(ad, key_added="other", switch_prob=1e-3)
    assert ad.uns["other"] == {"params": default_params, "planes": ["neutral"]} and len(default_params["levels"]) == 6
    assert np.array_equal(_bits(ad.obsm["X_other_neutral"]), _bits(default[2])) and "X_other_gain1" not in ad.obsm
    # device input leaves CUDA tensors
    ad = _adata(torch.from_numpy(x.toarray()).cuda(), pos)
    cnv.tl.cnv_copy_posteriors(ad, all_states=True, **kw)
    for name, ref in zip(names, want):
        got = ad.obsm[f"X_cnv_copy_posterior_{name}"]
        assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(_bits(got.cpu().numpy()), _bits(ref)), name


def test_all_zero_matrix_is_all_neutral_without_a_launch(monkeypatch):
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    launched = []
    monkeypatch.setattr(_engine, "copy_posterior_chains", lambda *a, **k: launched.append(1))
    pos = {"chr1": 0, "chr2": 17}
    for x in (sp.csr_matrix((5, 40)), np.zeros((5, 40), dtype=np.float32), torch.zeros((5, 40), device="cuda")):
        for kw in ({}, {"levels": (-1.0, 0.0, 1.0, 2.0)}):
            planes, info = _run(x, pos, all_states=True, return_info=True, **kw)
            z = info["neutral"]
            planes = [v.cpu().numpy() if torch.is_tensor(v) else v for v in planes]
            assert len(planes) == (4 if kw else 6) and info["sigma"] == 0.0
            for s, plane in enumerate(planes):
                assert plane.shape == (5, 40) and plane.dtype == np.float64 and (plane == (1.0 if s == z else 0.0)).all()
    # the zero model that tl.cnv_copy_states stored
    ad = _adata(sp.csr_matrix((5, 40)), pos)
    monkeypatch.setattr(_engine, "copy_states_viterbi", lambda *a, **k: launched.append(1))
    cnv.tl.cnv_copy_states(ad)
    assert ad.uns["cnv_copy_states"]["params"]["sigma"] == 0.0
    cnv.tl.cnv_copy_posteriors(ad, all_states=True)
    assert (ad.obsm["X_cnv_copy_posterior_neutral"] == 1.0).all() and not ad.obsm["X_cnv_copy_posterior_gain3"].any()
    assert ad.uns["cnv_copy_posterior"]["planes"] == ["loss2", "loss1", "neutral", "gain1", "gain2", "gain3"]
    assert not launched


def test_nonfinite_and_overflowing_values_raise_and_nothing_is_launched(monkeypatch):
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    launched = []
    real = _engine.copy_posterior_chains
    monkeypatch.setattr(_engine, "copy_posterior_chains", lambda *a, **k: launched.append(1) or real(*a, **k))
    c = so.planted(40, [20, 9], 5)
    pos = c["chr_pos"]
    for bad in (np.nan, np.inf, -np.inf):
        x = c["x"].copy()
        x.data[x.indptr[17]] = bad
        for kw in ({}, {"sigma": 0.2, "levels": (-0.4, 0.0, 0.4, 0.8)}):
            ad = _adata(x, pos)
            with pytest.raises(ValueError, match="non-finite"):
                cnv.tl.cnv_copy_posteriors(ad, **kw)
            assert "X_cnv_copy_posterior_neutral" not in ad.obsm and "cnv_copy_posterior" not in ad.uns
    x, pos1, kw = so.overflow_case()
    mu = [-0.2, 0.0, 0.2, 0.4]
    for sign in (1.0, -1.0):
        with pytest.raises(ValueError, match="overflow"):
            _run(sign * x, pos1, levels=mu, sigma=kw["sigma"])
        with pytest.raises(ValueError, match="overflow"):
            _run(sign * x, pos1, amplitude=0.2, sigma=kw["sigma"])  # the default levels reach 3 x 0.2
    assert not launched
    m = co.largest_value_that_does_not_overflow(mu, kw["sigma"])
    fine = x.copy()
    fine.data[fine.data == 1e160] = m
    planes = _run(fine, pos1, levels=mu, sigma=kw["sigma"], all_states=True)
    want, _ = cpo.cnv_copy_posteriors(fine, pos1, levels=mu, sigma=kw["sigma"])
    assert launched == [1] and all(np.array_equal(_bits(g), _bits(r)) for g, r in zip(planes, want))
    fine.data[fine.data == m] = float(np.nextafter(m, np.inf))
    with pytest.raises(ValueError, match="overflow"):
        _run(fine, pos1, levels=mu, sigma=kw["sigma"])
    assert launched == [1]


# ---- the filter --------------------------------------------------------------------------------------------------------------
def _filter_adata(states, p, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((states.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv_copy_states"] = states
    ad.obsm["X_cnv_copy_posterior_neutral"] = p
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _check_filter(states, p, chr_pos, max_p_normal=0.5):
    """tl.cnv_copy_states_filter equals the oracle; returns (filtered, removed)."""
    import infercnvpy_amd as cnv

    want, want_sign, want_fraction, want_removed, _ = cpo.copy_states_filter(states, p, chr_pos, max_p_normal)
    got, sign, fraction, removed = cnv.tl.cnv_copy_states_filter(_filter_adata(states, p, chr_pos), inplace=False,
                                                                 max_p_normal=max_p_normal)
    for plane in (got, sign):
        assert isinstance(plane, np.ndarray) and plane.dtype == np.int8 and plane.shape == states.shape
    assert fraction.dtype == np.float64 and removed.dtype == np.int32
    print(f"{states.shape}: {int((got != want).sum())} / {int((sign != want_sign).sum())} bytes of the two planes differ "
          f"from the oracle, {int(want_removed.sum())} runs removed")
    assert np.array_equal(got, want) and np.array_equal(sign, want_sign) and np.array_equal(sign, np.sign(got))
    assert np.array_equal(fraction, want_fraction) and np.array_equal(removed, want_removed)
    return got, removed


def _check_against_three_state_kernel(states, p, chr_pos, max_p_normal):
    """On calls in -1 / 0 / +1 icv_copy_states_filter gives the bytes of icv_states_filter."""
    import torch

    from infercnvpy_amd import _engine
    from infercnvpy_amd.tl._hmm import chromosome_bounds

    assert np.abs(states).max() <= 1
    bounds = chromosome_bounds(chr_pos, states.shape[1])
    s_dev = torch.from_numpy(np.array(states, dtype=np.int8)).cuda()  # (a copy: the cached cases are read-only)
    p_dev = torch.from_numpy(np.array(p, dtype=np.float64)).cuda()
    ref, ref_count, ref_removed, ref_bad = _engine.states_filter(s_dev, p_dev, bounds, max_p_normal)
    got, sign, count, removed, bad = _engine.copy_states_filter(s_dev, p_dev, bounds, max_p_normal)
    assert got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes() == sign.cpu().numpy().tobytes()
    assert torch.equal(count, ref_count) and torch.equal(removed, ref_removed)
    assert int(bad.item()) == int(ref_bad.item()) == 0
    return int(removed.sum().item())


@pytest.mark.parametrize("neighbourhood", po.SWEEP_NEIGHBOURHOODS)
def test_filter_step_boundary_sweeps_on_calls_doubled_calls_and_alternating_levels(neighbourhood):
    removed = 0
    for c in po.sweep_cases(neighbourhood):
        removed += _check_against_three_state_kernel(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])
        _check_filter(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])
        d = cpo.doubled(c)
        got, _ = _check_filter(d["states"], d["p"], d["chr_pos"], d["max_p_normal"])
        assert set(np.unique(got)) <= {-2, 0, 2}
        a = cpo.alternating(c)
        _check_filter(a["states"], a["p"], a["chr_pos"], a["max_p_normal"])
    assert removed > 50


def test_filter_half_integer_and_big_sum_cases_on_calls_and_doubled_calls():
    c = po.half_integer_case()
    assert _check_against_three_state_kernel(c["states"], c["p"], c["chr_pos"], c["max_p_normal"]) == 7
    for case in (c, cpo.doubled(c)):
        got, removed = _check_filter(case["states"], case["p"], case["chr_pos"], case["max_p_normal"])
        assert removed.tolist() == [0, 0, 7] and np.array_equal(got[0], case["states"][0])
    c = po.big_sum_case()
    d = cpo.doubled(c)
    for i, mean in enumerate(c["means"]):
        below = float(np.nextafter(mean, 0.0))
        _check_against_three_state_kernel(c["states"], c["p"], c["chr_pos"], mean)
        _check_against_three_state_kernel(c["states"], c["p"], c["chr_pos"], below)
        got, removed = _check_filter(d["states"], d["p"], d["chr_pos"], mean)
        assert got[i].any() and removed[i] == 0
        got, removed = _check_filter(d["states"], d["p"], d["chr_pos"], below)
        assert not got[i].any() and removed[i] == 1


@pytest.mark.parametrize("name", list(cpo.crafted_filter_cases()))
def test_filter_crafted_verdicts(name):
    c = cpo.crafted_filter_cases()[name]
    got, _ = _check_filter(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])
    assert np.array_equal(got, c["want"])


def test_filter_refuses_levels_beyond_seven_and_bad_posteriors():
    import infercnvpy_amd as cnv

    states, p = po.random_calls(9, [50, 51], seed=3)
    pos = {"a": 0, "b": 50}
    for level in (8, -8):
        bad = (states * 3).astype(np.int8)
        bad[4, 70] = level
        with pytest.raises(ValueError, match=r"levels outside \[-7, 7\]"):
            cnv.tl.cnv_copy_states_filter(_filter_adata(bad, p, pos))
    for value in (np.nan, 1.5, -0.25):
        q = p.copy()
        q[6, 3] = value
        with pytest.raises(ValueError, match="not numbers in"):
            cnv.tl.cnv_copy_states_filter(_filter_adata(states, q, pos))
    edge = (states * 7).astype(np.int8)
    got, _ = _check_filter(edge, p, pos)
    assert set(np.unique(got)) == {-7, 0, 7}


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def test_chain_from_the_calls_to_the_segment_table_on_the_planted_case():
    import infercnvpy_amd as cnv

    c = cpo.chain_case()
    ad = _adata(c["x"], c["chr_pos"])
    cnv.tl.cnv_copy_states(ad, **c["kwargs"])
    cnv.tl.cnv_copy_posteriors(ad)
    assert np.array_equal(ad.obsm["X_cnv_copy_states"], c["states"])
    assert np.array_equal(_bits(ad.obsm["X_cnv_copy_posterior_neutral"]), _bits(c["neutral"]))
    assert cnv.tl.cnv_copy_states_filter(ad, max_p_normal=cpo.CHAIN_MAX_P_NORMAL) is None
    assert ad.obsm["X_cnv_copy_states_filtered"].tobytes() == c["filtered"].tobytes()
    assert ad.obsm["X_cnv_copy_states_filtered_sign"].tobytes() == c["sign"].tobytes()
    assert np.array_equal(ad.obs["cnv_copy_states_filtered_fraction"].to_numpy(), c["fraction"])
    removed = ad.obs["cnv_copy_states_filtered_removed"].to_numpy()
    assert np.array_equal(removed, c["removed"]) and int(removed.sum()) == 2
    assert ad.uns["cnv_copy_states_filtered"] == {
        "params": {"max_p_normal": cpo.CHAIN_MAX_P_NORMAL, "use_rep": "cnv_copy_states",
                   "posterior_key": "cnv_copy_posterior"}, "chr_pos": dict(c["chr_pos"])}
    assert ad.uns["cnv_copy_states_filtered"]["chr_pos"] is not ad.uns["cnv"]["chr_pos"]  # a copy
    wrong = int((ad.obsm["X_cnv_copy_states_filtered"] != c["truth"]).sum())
    print(f"wrong calls of {c['truth'].size}: {int((c['states'] != c['truth']).sum())} before the filter, {wrong} after")
    assert wrong == cpo.CHAIN_WRONG_AFTER
    table = cnv.tl.cnv_segments(ad, use_rep="cnv_copy_states_filtered_sign", groupby=None, inplace=False)
    want = sg.segments(c["sign"], sg.bounds(c["chr_pos"], c["x"].shape[1]))
    assert want["row"].shape[0] >= 4 * 24
    for k, col in zip(("row", "start", "end", "state"), ("cell", "start", "end", "state")):
        assert np.array_equal(table[col].to_numpy(), want[k]), col
    _, _, _, _, info = cnv.tl.cnv_copy_states_filter(ad, max_p_normal=cpo.CHAIN_MAX_P_NORMAL, inplace=False,
                                                     return_info=True)
    assert info["n_removed"] == 2 and set(info["stage_ms"]) == {"filter"}

"""tl.cnv_copy_states on the GPU equals the oracle of DESIGN.md 4.22 (tests/_copy_states_oracle.py) byte for byte, and with
three levels the bytes of tl.cnv_states: every K and neutral position, the rounding case, every chromosome layout and
output split, every kind of input, the defaults, the planted multi-level case and the errors that need the device."""
import numpy as np
import pytest
import scipy.sparse as sp

import _copy_states_oracle as co
import _segments_oracle as sg
import _states_oracle as so

pytestmark = pytest.mark.gpu


def _adata(x, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _run(x, chr_pos, **kw):
    import infercnvpy_amd as cnv

    return cnv.tl.cnv_copy_states(_adata(x, chr_pos), inplace=False, **kw)


def _check_case(name):
    c = co.case(name)
    states, sign, fraction = _run(c["x"], c["chr_pos"], **c["kwargs"])
    for got in (states, sign):
        assert isinstance(got, np.ndarray) and got.dtype == np.int8 and got.shape == c["x"].shape
    assert isinstance(fraction, np.ndarray) and fraction.dtype == np.float64
    print(f"{name}: {c['x'].shape}, {int((states != c['states']).sum())} / {int((sign != c['sign']).sum())} bytes of the "
          "two planes differ from the oracle")
    assert np.array_equal(states, c["states"])
    assert np.array_equal(sign, c["sign"])
    assert np.array_equal(fraction, c["fraction"])
    return c


TIES_HIGH_SWITCH = "ties_switch_0.9"  # above (K - 1) / K = 2 / 3: leaving costs less than staying, a2 / m2 decide
THREE_STATE_CASES = (["ties", "rounding_ties", "planted777", "full_and_empty"]
                     + [f"output_split_{w}" for w in so.SPLIT_WIDTHS] + [TIES_HIGH_SWITCH])


def _three_state_case(name):
    """``_states_oracle.case(name)``; TIES_HIGH_SWITCH is its ``ties`` matrix called at switch_prob = 0.9."""
    if name != TIES_HIGH_SWITCH:
        return so.case(name)
    c = so.ties()
    c["kwargs"]["switch_prob"] = 0.9
    c["states"], c["fraction"], c["params"] = so.cnv_states(c["x"], c["chr_pos"], **c["kwargs"])
    assert c["params"]["switch_prob"] == 0.9 and (c["states"] != so.case("ties")["states"]).mean() > 0.25
    return c


@pytest.mark.parametrize("name", THREE_STATE_CASES)
def test_three_levels_give_the_bytes_of_cnv_states(name):
    import infercnvpy_amd as cnv

    c = _three_state_case(name)
    a, sigma, p = c["params"]["amplitude"], c["params"]["sigma"], c["params"]["switch_prob"]
    three, three_fraction = cnv.tl.cnv_states(_adata(c["x"], c["chr_pos"]), inplace=False, amplitude=a, sigma=sigma,
                                              switch_prob=p)
    states, sign, fraction = _run(c["x"], c["chr_pos"], levels=(-a, 0.0, a), sigma=sigma, switch_prob=p)
    print(f"{name}: {int((states != three).sum())} bytes differ from tl.cnv_states, {int((states != c['states']).sum())} "
          "from the states oracle")
    assert states.tobytes() == three.tobytes() == c["states"].tobytes()
    assert sign.tobytes() == states.tobytes()
    assert fraction.tobytes() == three_fraction.tobytes() == c["fraction"].tobytes()


@pytest.mark.parametrize("k", range(co.MIN_STATES, co.MAX_STATES + 1))
def test_every_k_and_neutral_position_equals_the_oracle(k):
    for z in range(k):
        for p in co.EVERY_K_SWITCH:
            c = _check_case(f"every_k_{k}_{z}_{p}")
            assert 30 <= c["x"].shape[0] <= 45 and not c["states"][-1].any()
            if k == 6:
                assert set(np.unique(c["states"])) == set(range(-z, k - z)), (z, p)  # every level occurs


def test_rounding_case_equals_the_oracle():
    c = _check_case("rounding_ties")
    assert c["x"].shape == (co.ROUNDING_ROWS, 1100) and len(c["chr_pos"]) == 300


@pytest.mark.parametrize("name", co.SHAPE_NAMES)
def test_every_chromosome_layout_equals_the_oracle(name):
    c = _check_case(name)
    if name == "max_windows":
        assert c["x"].shape == (2, co.MAX_WINDOWS) and len(set(np.diff(so.bounds(c["chr_pos"], co.MAX_WINDOWS)))) == 3


@pytest.mark.parametrize("w", so.SPLIT_WIDTHS)
def test_both_planes_take_every_head_word_and_tail_split(w):
    c = _check_case(f"output_split_{w}")
    st = c["states"]
    offsets = {(i * w) % 4 for i in range(so.SPLIT_ROWS)}
    ends = {(i * w) % 4 for i in range(so.SPLIT_ROWS) if st[i, 0] != 0 and st[i, -1] != 0}
    assert ends == offsets and (st != 0).mean() > 0.5
    assert w < 4 or (st != c["sign"]).any()  # the planes differ: one written in the other's place would show


def test_every_kind_of_input_gives_the_same_bytes():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(150, [33, 1, 70, 7], 21)
    dense32 = c["x"].toarray().astype(np.float32)  # float32 numbers: exactly representable in every form below
    x = sp.csr_matrix(dense32.astype(np.float64))
    pos = c["chr_pos"]
    kw = {"amplitude": 0.3, "sigma": 0.1}
    want, want_sign, want_fraction, params = co.cnv_copy_states(x, pos, **kw)
    assert set(np.unique(want)) >= {-2, -1, 0, 1, 2}
    dev_csr = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                            torch.from_numpy(x.indices.astype(np.int32)).cuda(), torch.from_numpy(x.data).cuda(),
                            x.shape[1])
    inputs = {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
              "dense_float64": dense32.astype(np.float64), "packed_csr": dev_csr,
              "cuda_float32": torch.from_numpy(dense32).cuda(), "cuda_float64": torch.from_numpy(dense32).cuda().double()}
    for name, xin in inputs.items():
        states, sign, fraction, info = _run(xin, pos, return_info=True, **kw)
        on_device = name in ("packed_csr", "cuda_float32", "cuda_float64")
        assert all(torch.is_tensor(v) == on_device for v in (states, sign, fraction)), name
        if on_device:
            assert states.is_cuda and states.dtype == torch.int8 and sign.is_cuda and sign.dtype == torch.int8
            assert fraction.is_cuda and fraction.dtype == torch.float64
            states, sign, fraction = states.cpu().numpy(), sign.cpu().numpy(), fraction.cpu().numpy()
        assert info["levels"] == params["levels"] and info["neutral"] == 2 and info["sigma"] == 0.1, name
        assert info["n_chromosomes"] == 4 and set(info["stage_ms"]) == {"rowsq", "viterbi"}
        assert np.array_equal(states, want), name
        assert np.array_equal(sign, want_sign), name
        assert np.array_equal(fraction, want_fraction), name


def test_defaults_and_inplace_results():
    import torch

    import infercnvpy_amd as cnv

    c = so.case("one_window_chromosome_between_long")
    x, pos = c["x"], c["chr_pos"]
    want, want_sign, want_fraction, params = co.cnv_copy_states(x, pos)
    sigma = so.default_sigma(x)
    assert params["sigma"] == sigma and params["levels"] == [float(k) * (2.0 * sigma) for k in (-2, -1, 0, 1, 2, 3)]
    ad = _adata(x, pos)
    assert cnv.tl.cnv_copy_states(ad) is None
    for key, plane in (("X_cnv_copy_states", want), ("X_cnv_copy_states_sign", want_sign)):
        assert isinstance(ad.obsm[key], np.ndarray) and ad.obsm[key].dtype == np.int8 and np.array_equal(ad.obsm[key], plane)
    assert np.array_equal(ad.obs["cnv_copy_states_fraction"].to_numpy(), want_fraction)
    assert ad.uns["cnv_copy_states"] == {"params": params, "chr_pos": dict(pos)}
    assert ad.uns["cnv_copy_states"]["params"]["switch_prob"] == 1e-3 and ad.uns["cnv_copy_states"]["params"]["neutral"] == 2
    assert ad.uns["cnv_copy_states"]["chr_pos"] is not ad.uns["cnv"]["chr_pos"]  # a copy
    _, _, _, info = _run(x, pos, return_info=True)
    assert info["sigma"] == sigma and info["levels"] == params["levels"]
    ad = _adata(torch.from_numpy(x.toarray()).cuda(), pos)
    cnv.tl.cnv_copy_states(ad, key_added="levels", levels=params["levels"], sigma=sigma)
    assert ad.obsm["X_levels"].is_cuda and np.array_equal(ad.obsm["X_levels"].cpu().numpy(), want)
    assert ad.obsm["X_levels_sign"].is_cuda and np.array_equal(ad.obsm["X_levels_sign"].cpu().numpy(), want_sign)
    assert np.array_equal(ad.obs["levels_fraction"].to_numpy(), want_fraction)


def test_planted_levels_on_the_gpu_and_their_segments():
    import infercnvpy_amd as cnv

    for seed in range(5):
        c = _check_case(f"planted_levels_{seed}")
        wrong6 = int((c["states"] != c["truth"]).sum())
        three, _, _ = so.cnv_states(c["x"], c["chr_pos"], amplitude=0.3, sigma=0.1)
        wrong3 = int((three != c["truth"]).sum())
        print(f"seed {seed}: wrong calls of {c['truth'].size}: six states {wrong6}, three states {wrong3}")
        assert wrong6 <= co.PLANTED_MOST_WRONG and wrong3 >= co.PLANTED_LEAST_WRONG
    c = co.case("planted_levels_0")
    ad = _adata(c["x"], c["chr_pos"])
    cnv.tl.cnv_copy_states(ad, **c["kwargs"])
    table = cnv.tl.cnv_segments(ad, use_rep="cnv_copy_states_sign", groupby=None, inplace=False)
    want = sg.segments(c["sign"], sg.bounds(c["chr_pos"], c["x"].shape[1]))
    assert want["row"].shape[0] >= 4 * 24
    for k, col in zip(("row", "start", "end", "state"), ("cell", "start", "end", "state")):
        assert np.array_equal(table[col].to_numpy(), want[k]), col
    assert np.array_equal(table["n_windows"].to_numpy(), want["end"] - want["start"])


def test_nonfinite_and_overflowing_values_raise_and_nothing_is_launched(monkeypatch):
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    launched = []
    real = _engine.copy_states_viterbi
    monkeypatch.setattr(_engine, "copy_states_viterbi", lambda *a, **k: launched.append(1) or real(*a, **k))
    c = so.planted(40, [20, 9], 5)
    pos = c["chr_pos"]
    for bad in (np.nan, np.inf, -np.inf):
        x = c["x"].copy()
        x.data[x.indptr[17]] = bad
        for kw in ({}, {"sigma": 0.2, "levels": (-0.4, 0.0, 0.4, 0.8)}):
            ad = _adata(x, pos)
            with pytest.raises(ValueError, match="non-finite"):
                cnv.tl.cnv_copy_states(ad, **kw)
            assert "X_cnv_copy_states" not in ad.obsm and "cnv_copy_states" not in ad.uns
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
    states, sign_plane, _ = _run(fine, pos1, levels=mu, sigma=kw["sigma"])
    want = co.cnv_copy_states(fine, pos1, levels=mu, sigma=kw["sigma"])
    assert launched == [1] and np.array_equal(states, want[0]) and np.array_equal(sign_plane, want[1])
    fine.data[fine.data == m] = float(np.nextafter(m, np.inf))
    with pytest.raises(ValueError, match="overflow"):
        _run(fine, pos1, levels=mu, sigma=kw["sigma"])
    assert launched == [1]


def test_all_zero_matrix_is_all_neutral_without_a_launch(monkeypatch):
    import torch

    from infercnvpy_amd import _engine

    launched = []
    monkeypatch.setattr(_engine, "copy_states_viterbi", lambda *a, **k: launched.append(1))
    pos = {"chr1": 0, "chr2": 17}
    for x in (sp.csr_matrix((5, 40)), np.zeros((5, 40), dtype=np.float32), torch.zeros((5, 40), device="cuda")):
        for kw in ({}, {"levels": (-1.0, 0.0, 1.0, 2.0)}):
            states, sign, fraction, info = _run(x, pos, return_info=True, **kw)
            if torch.is_tensor(states):
                states, sign, fraction = states.cpu().numpy(), sign.cpu().numpy(), fraction.cpu().numpy()
            for plane in (states, sign):
                assert plane.shape == (5, 40) and plane.dtype == np.int8 and not plane.any()
            assert not fraction.any() and info["sigma"] == 0.0
    assert not launched

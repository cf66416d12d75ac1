"""tl.cnv_states on the GPU equals the oracle of DESIGN.md 4.13 (tests/_states_oracle.py) byte for byte: every
chromosome layout, the tie rules, every kind of input, the default sigma, boundaries and the non-finite check."""
import numpy as np
import pytest
import scipy.sparse as sp

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

    return cnv.tl.cnv_states(_adata(x, chr_pos), inplace=False, **kw)


def _check_case(name):
    c = so.case(name)
    states, fraction = _run(c["x"], c["chr_pos"], **c["kwargs"])
    assert isinstance(states, np.ndarray) and states.dtype == np.int8 and states.shape == c["x"].shape
    assert isinstance(fraction, np.ndarray) and fraction.dtype == np.float64
    diff = int((states != c["states"]).sum())
    print(f"{name}: {c['x'].shape}, {diff} bytes differ from the oracle")
    assert np.array_equal(states, c["states"])
    assert np.array_equal(fraction, c["fraction"])


@pytest.mark.parametrize("name", so.SHAPE_NAMES)
def test_every_chromosome_layout_equals_the_oracle(name):
    _check_case(name)


def test_tie_rules_equal_the_oracle():
    _check_case("ties")
    c = so.case("ties")
    assert (c["states"] == -1).any() and (c["states"] == 1).any() and not c["states"][-2].any()


def test_777_cells_equal_the_oracle():
    _check_case("planted777")


def test_full_rows_next_to_empty_rows_equal_the_oracle():
    c = so.case("full_and_empty")
    lens = np.diff(c["x"].indptr)
    assert lens.max() == c["x"].shape[1] and (lens == 0).sum() >= 3
    _check_case("full_and_empty")


def test_every_kind_of_input_gives_the_same_bytes():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(150, [33, 1, 70, 7], 21)
    dense32 = c["x"].toarray().astype(np.float32)  # float32 numbers: exactly representable in every form below
    x = sp.csr_matrix(dense32.astype(np.float64))
    pos = c["chr_pos"]
    want, want_fraction, params = so.cnv_states(x, pos)
    dev_csr = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                            torch.from_numpy(x.indices.astype(np.int32)).cuda(), torch.from_numpy(x.data).cuda(),
                            x.shape[1])
    inputs = {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
              "dense_float64": dense32.astype(np.float64), "packed_csr": dev_csr,
              "cuda_float32": torch.from_numpy(dense32).cuda(), "cuda_float64": torch.from_numpy(dense32).cuda().double()}
    for name, xin in inputs.items():
        states, fraction, info = _run(xin, pos, return_info=True)
        on_device = name in ("packed_csr", "cuda_float32", "cuda_float64")
        assert torch.is_tensor(states) == on_device and torch.is_tensor(fraction) == on_device, name
        if on_device:
            assert states.is_cuda and states.dtype == torch.int8 and fraction.is_cuda and fraction.dtype == torch.float64
            states, fraction = states.cpu().numpy(), fraction.cpu().numpy()
        assert info["sigma"] == params["sigma"] and info["amplitude"] == params["amplitude"], name  # == on float64
        assert info["n_chromosomes"] == 4 and set(info["stage_ms"]) == {"rowsq", "viterbi"}
        assert np.array_equal(states, want), name
        assert np.array_equal(fraction, want_fraction), name


def test_inplace_writes_obsm_obs_and_uns():
    import torch

    import infercnvpy_amd as cnv

    c = so.case("one_window_chromosome_between_long")
    ad = _adata(c["x"], c["chr_pos"])
    assert cnv.tl.cnv_states(ad) is None
    assert np.array_equal(ad.obsm["X_cnv_states"], c["states"]) and ad.obsm["X_cnv_states"].dtype == np.int8
    assert np.array_equal(ad.obs["cnv_states_fraction"].to_numpy(), c["fraction"])
    assert ad.uns["cnv_states"] == {"params": c["params"]}
    ad = _adata(torch.from_numpy(c["x"].toarray()).cuda(), c["chr_pos"])
    cnv.tl.cnv_states(ad, key_added="calls", amplitude=c["params"]["amplitude"], sigma=c["params"]["sigma"])
    assert ad.obsm["X_calls"].is_cuda and np.array_equal(ad.obsm["X_calls"].cpu().numpy(), c["states"])
    assert np.array_equal(ad.obs["calls_fraction"].to_numpy(), c["fraction"])


def test_default_sigma_equals_the_oracles():
    c = so.case("planted777")
    _, _, info = _run(c["x"], c["chr_pos"], return_info=True)
    assert info["sigma"] == so.default_sigma(c["x"]) == c["params"]["sigma"]
    assert info["amplitude"] == 2.0 * info["sigma"]


def test_all_zero_matrix_is_all_neutral():
    import torch

    pos = {"chr1": 0, "chr2": 17}
    for x in (sp.csr_matrix((5, 40)), np.zeros((5, 40), dtype=np.float32), torch.zeros((5, 40), device="cuda")):
        states, fraction, info = _run(x, pos, return_info=True)
        if torch.is_tensor(states):
            states, fraction = states.cpu().numpy(), fraction.cpu().numpy()
        assert states.shape == (5, 40) and states.dtype == np.int8 and not states.any() and not fraction.any()
        assert info["sigma"] == 0.0 and info["amplitude"] == 0.0


def test_second_call_gives_the_same_bytes():
    c = so.case("chromosomes_130")
    first = _run(c["x"], c["chr_pos"])
    second = _run(c["x"], c["chr_pos"])
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_chromosome_boundary_is_honoured():
    """A +a run ending on the last window of one chromosome and a -a run starting on the next one both survive with
    switch_prob=1e-12.  A switch then costs 28.3; a run of 16 windows is worth 16 a^2 h = 32 over neutral: enough for the
    one switch it needs inside its own chromosome (and cheaper than calling the 24 neutral windows beside it too: 48),
    not for the three switches both runs would need in ONE chain (64 < 84.9), where the same row stays neutral."""
    a, w, cut, run = 1.0, 80, 40, 16
    row = np.zeros(w)
    row[cut - run:cut] = a
    row[cut:cut + run] = -a
    x = sp.csr_matrix(np.vstack([row, -row, np.zeros(w)]))
    kw = {"amplitude": a, "sigma": 0.5, "switch_prob": 1e-12}
    pos = {"chr1": 0, "chr2": cut}
    states, fraction = _run(x, pos, **kw)
    want, want_fraction, _ = so.cnv_states(x, pos, **kw)
    assert np.array_equal(states, want) and np.array_equal(fraction, want_fraction)
    assert np.array_equal(states[0], np.sign(row)) and np.array_equal(states[1], -np.sign(row)) and not states[2].any()
    one, _ = _run(x, {"chr1": 0}, **kw)
    assert np.array_equal(one, so.cnv_states(x, {"chr1": 0}, **kw)[0]) and not one.any()


def test_nan_raises_and_nothing_is_launched_after_it(monkeypatch):
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    launched = []
    real = _engine.states_viterbi
    monkeypatch.setattr(_engine, "states_viterbi", lambda *a, **k: launched.append(1) or real(*a, **k))
    c = so.planted(40, [20, 9], 5)
    pos = c["chr_pos"]
    for bad in (np.nan, np.inf, -np.inf):
        x = c["x"].copy()
        x.data[x.indptr[17]] = bad
        for xin in (x, x.toarray(), torch.from_numpy(x.toarray()).cuda()):
            for kw in ({}, {"sigma": 0.2, "amplitude": 0.4}):
                ad = _adata(xin, pos)
                with pytest.raises(ValueError, match="non-finite"):
                    cnv.tl.cnv_states(ad, **kw)
                assert "X_cnv_states" not in ad.obsm and "cnv_states" not in ad.uns
    assert not launched
    states, _ = _run(c["x"], pos)  # the finite matrix still runs, through the same wrapper
    assert launched == [1] and states.shape == c["x"].shape


@pytest.mark.parametrize("w", [1, 3, 7, 111, 1802, so.MAX_WINDOWS])
def test_device_fraction_is_the_hosts_division(w):
    """Every count 0 .. W over W: the device's quotient has the bits of the host's float64 division (a product with
    1 / W does not)."""
    import torch

    from infercnvpy_amd import _engine

    counts = np.arange(w + 1, dtype=np.int32)
    got = _engine.states_fraction(torch.from_numpy(counts).cuda(), w)
    assert got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), counts.astype(np.float64) / float(w))

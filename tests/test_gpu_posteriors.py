"""tl.cnv_posteriors on the GPU equals the oracle of DESIGN.md 4.15 (tests/_posterior_oracle.py) on the float64 bytes:
every chromosome layout, the window cap, exact zeros and ones, every switch probability, every kind of input, the
parameters of tl.cnv_states, the all-zero matrix and the non-finite check."""
import numpy as np
import pytest
import scipy.sparse as sp

import _posterior_oracle as po
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

    return cnv.tl.cnv_posteriors(_adata(x, chr_pos), inplace=False, **kw)


def _same(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape, what
    differ = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    worst = float(np.nanmax(np.abs(got - want))) if differ else 0.0
    print(f"{what}: {want.shape}, {differ} values differ from the oracle, largest difference {worst:.3g}")
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("name", po.CASE_NAMES)
def test_every_case_equals_the_oracle(name):
    c = po.case(name)
    neutral = _run(c["x"], c["chr_pos"], **c["kwargs"])
    _same(neutral, c["neutral"], name + " neutral")
    loss, neutral3, gain = _run(c["x"], c["chr_pos"], all_states=True, **c["kwargs"])
    _same(neutral3, c["neutral"], name + " neutral of three")
    _same(loss, c["loss"], name + " loss")
    _same(gain, c["gain"], name + " gain")


def test_the_cases_are_what_they_are_meant_to_be():
    assert po.case("one_window")["x"].shape[1] == 1
    w = po.case("odd_width")["x"].shape[1]
    assert w % 4 and w % 64
    assert len(po.case("chromosomes_65")["chr_pos"]) == 65 and len(po.case("chromosomes_130")["chr_pos"]) == 130
    c = po.case("max_windows")
    assert c["x"].shape == (3, po.MAX_WINDOWS) and len(c["chr_pos"]) == 1
    assert po.case("planted300")["x"].shape == (300, 1802) and len(po.case("planted300")["chr_pos"]) == 23
    lens = np.diff(po.case("full_and_empty")["x"].indptr)
    assert lens.max() == po.case("full_and_empty")["x"].shape[1] and (lens == 0).sum() >= 3
    c = po.case("outliers")
    assert (c["gain"] == 1.0).any() and (c["loss"] == 1.0).any() and (c["neutral"] == 0.0).any()


def test_one_window_above_the_cap_raises():
    import infercnvpy_amd as cnv

    ad = _adata(sp.csr_matrix((2, po.MAX_WINDOWS + 1)), {"chr1": 0})
    with pytest.raises(ValueError, match=str(po.MAX_WINDOWS)):
        cnv.tl.cnv_posteriors(ad)


def test_every_kind_of_input_gives_the_same_bytes():
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(150, [33, 1, 70, 7], 21)
    dense32 = c["x"].toarray().astype(np.float32)  # float32 numbers: exactly representable in every form below
    x = sp.csr_matrix(dense32.astype(np.float64))
    pos = c["chr_pos"]
    wl, wn, wg, params = po.cnv_posteriors(x, pos)
    dev_csr = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                            torch.from_numpy(x.indices.astype(np.int32)).cuda(), torch.from_numpy(x.data).cuda(),
                            x.shape[1])
    inputs = {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
              "dense_float64": dense32.astype(np.float64), "packed_csr": dev_csr,
              "cuda_float32": torch.from_numpy(dense32).cuda(), "cuda_float64": torch.from_numpy(dense32).cuda().double()}
    host = _run(x, pos, all_states=True)
    for name, xin in inputs.items():
        (loss, neutral, gain), info = _run(xin, pos, all_states=True, return_info=True)
        on_device = name in ("packed_csr", "cuda_float32", "cuda_float64")
        for v in (loss, neutral, gain):
            assert torch.is_tensor(v) == on_device, name
            if on_device:
                assert v.is_cuda and v.dtype == torch.float64
        if on_device:
            loss, neutral, gain = (v.cpu().numpy() for v in (loss, neutral, gain))
        assert info["sigma"] == params["sigma"] and info["amplitude"] == params["amplitude"], name
        assert info["switch_prob"] == 1e-3 and info["n_chromosomes"] == 4 and set(info["stage_ms"]) == {"rowsq", "chains"}
        for got, first, want in zip((loss, neutral, gain), host, (wl, wn, wg)):
            assert got.tobytes() == first.tobytes(), name
            assert np.array_equal(got, want), name


def test_parameters_come_from_cnv_states_and_keywords_override_them():
    import infercnvpy_amd as cnv

    c = so.planted(30, [20, 3, 14], 17)
    ad = _adata(c["x"], c["chr_pos"])
    cnv.tl.cnv_states(ad, amplitude=0.25, sigma=0.125, switch_prob=0.01)
    assert cnv.tl.cnv_posteriors(ad) is None
    want = po.cnv_posteriors(c["x"], c["chr_pos"], amplitude=0.25, sigma=0.125, switch_prob=0.01)
    assert ad.uns["cnv_posterior"] == {"params": want[3]} == {"params": ad.uns["cnv_states"]["params"]}
    assert np.array_equal(ad.obsm["X_cnv_posterior_neutral"], want[1])
    assert "X_cnv_posterior_loss" not in ad.obsm and "X_cnv_posterior_gain" not in ad.obsm
    # one explicit keyword: the other two resolve as in tl.cnv_states, not from uns
    cnv.tl.cnv_posteriors(ad, key_added="mine", switch_prob=0.3, all_states=True)
    want = po.cnv_posteriors(c["x"], c["chr_pos"], switch_prob=0.3)
    assert ad.uns["mine"]["params"] == want[3] and want[3]["sigma"] == so.default_sigma(c["x"])
    for k, v in zip(("loss", "neutral", "gain"), want[:3]):
        assert np.array_equal(ad.obsm[f"X_mine_{k}"], v), k
    # no tl.cnv_states result under states_key: the defaults
    cnv.tl.cnv_posteriors(ad, key_added="plain", states_key="nothing_here")
    assert np.array_equal(ad.obsm["X_plain_neutral"], po.cnv_posteriors(c["x"], c["chr_pos"])[1])


def test_device_input_stays_on_the_device_in_place():
    import torch

    import infercnvpy_amd as cnv

    c = po.case("short_chromosomes")
    ad = _adata(torch.from_numpy(c["x"].toarray()).cuda(), c["chr_pos"])
    cnv.tl.cnv_posteriors(ad, all_states=True)
    for k in ("loss", "neutral", "gain"):
        v = ad.obsm[f"X_cnv_posterior_{k}"]
        assert v.is_cuda and v.dtype == torch.float64 and np.array_equal(v.cpu().numpy(), c[k])


def test_all_zero_matrix_is_neutral():
    import torch

    import infercnvpy_amd as cnv

    pos = {"chr1": 0, "chr2": 17}
    for x in (sp.csr_matrix((5, 40)), np.zeros((5, 40), dtype=np.float32), torch.zeros((5, 40), device="cuda")):
        (loss, neutral, gain), info = _run(x, pos, all_states=True, return_info=True)
        if torch.is_tensor(neutral):
            loss, neutral, gain = (v.cpu().numpy() for v in (loss, neutral, gain))
        assert neutral.shape == (5, 40) and neutral.dtype == np.float64
        assert (neutral == 1.0).all() and not loss.any() and not gain.any() and info["sigma"] == 0.0
    ad = _adata(sp.csr_matrix((5, 40)), pos)  # and after tl.cnv_states left sigma = 0 in uns
    cnv.tl.cnv_states(ad)
    cnv.tl.cnv_posteriors(ad)
    assert (ad.obsm["X_cnv_posterior_neutral"] == 1.0).all()


def test_nan_and_inf_raise_and_nothing_is_launched(monkeypatch):
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    launched = []
    real = _engine.posterior_chains
    monkeypatch.setattr(_engine, "posterior_chains", lambda *a, **k: launched.append(1) or real(*a, **k))
    c = so.planted(40, [20, 9], 5)
    pos = c["chr_pos"]
    for bad in (np.nan, np.inf, -np.inf):
        x = c["x"].copy()
        x.data[x.indptr[17]] = bad
        for xin in (x, x.toarray(), torch.from_numpy(x.toarray()).cuda()):
            for kw in ({}, {"sigma": 0.2, "amplitude": 0.4}):
                ad = _adata(xin, pos)
                with pytest.raises(ValueError, match="non-finite"):
                    cnv.tl.cnv_posteriors(ad, **kw)
                assert "X_cnv_posterior_neutral" not in ad.obsm and "cnv_posterior" not in ad.uns
    assert not launched
    assert _run(c["x"], pos).shape == c["x"].shape and launched == [1]


def test_second_call_gives_the_same_bytes():
    c = po.case("chromosomes_130")
    first = _run(c["x"], c["chr_pos"], all_states=True)
    second = _run(c["x"], c["chr_pos"], all_states=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))


def test_called_windows_are_unlikely_to_be_neutral():
    import infercnvpy_amd as cnv

    c = po.case("planted300")
    ad = _adata(c["x"], c["chr_pos"])
    cnv.tl.cnv_states(ad)
    cnv.tl.cnv_posteriors(ad)
    called = ad.obsm["X_cnv_states"] != 0
    median = float(np.median(ad.obsm["X_cnv_posterior_neutral"][called]))
    print(f"{int(called.sum())} windows called, median P(neutral) = {median:.3g}")
    assert called.sum() > 1000 and median < 0.5

"""tl.cnv_states at the limits of k_states_viterbi ("limits pinned"): chains whose call the last bit of
a sum decides, the int8 row's head / word / tail split at every width and row offset, dense input with a leading
dimension above W, chr_start layouts that only the C ABI reaches, and the emission overflow check."""
import numpy as np
import pytest
import scipy.sparse as sp

import _states_oracle as so

pytestmark = pytest.mark.gpu

PADS = (1, 64)
PAD_VALUE = 1e30  # finite in float32 and float64: a kernel that reads the padding changes every result


def _adata(x, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _run(x, chr_pos, **kw):
    import infercnvpy_amd as cnv

    return cnv.tl.cnv_states(_adata(x, chr_pos), inplace=False, **kw)


def _same_calls(got, fraction, c, what):
    assert isinstance(got, np.ndarray) and got.dtype == np.int8 and got.shape == c["states"].shape, what
    print(f"{what}: {got.shape}, {int((got != c['states']).sum())} bytes differ from the oracle")
    assert got.tobytes() == c["states"].tobytes(), what
    assert fraction.tobytes() == c["fraction"].tobytes(), what


# ---- A: the order of the operations of rules 2-3 ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["csr_float64", "dense_float64"])
def test_rounding_decided_ties_equal_the_contract(kind):
    """tests/test_states_oracle.py shows that d + (T + e), -(t (t h)) and a fused -(t t) h + best each change the calls of
    at least 27 of the 400 chains of every length: equal bytes mean the kernel evaluates rules 2-3 as written."""
    c = so.case("rounding_ties")
    x = c["x"] if kind == "csr_float64" else c["x"].toarray()
    states, fraction = _run(x, c["chr_pos"], **c["kwargs"])
    _same_calls(states, fraction, c, kind)


# ---- B: the int8 row leaves as head bytes, 4-byte words and tail bytes ---------------------------------------------------------
@pytest.mark.parametrize("w", so.SPLIT_WIDTHS)
def test_output_split_at_every_width_and_row_offset(w):
    c = so.case(f"output_split_{w}")
    states, fraction = _run(c["x"], c["chr_pos"], **c["kwargs"])
    _same_calls(states, fraction, c, f"W = {w}")


# ---- B: dense input whose rows are further apart than W -----------------------------------------------------------------------
def _padded(dense, pad, dtype):
    import torch

    from infercnvpy_amd import _engine

    n, w = dense.shape
    buf = torch.full((n, w + pad), PAD_VALUE, dtype=dtype, device="cuda")
    buf[:, :w] = torch.from_numpy(dense).cuda().to(dtype)
    dm = _engine.DeviceMatrix(dense=buf[:, :w])
    assert dm.c_struct().ld == w + pad
    return dm


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_padded_dense_rows_equal_the_contiguous_matrix_and_the_oracle(dtype):
    import torch

    from infercnvpy_amd import _engine
    from infercnvpy_amd.tl._states import chromosome_bounds

    c = so.planted(13, [33, 1, 70, 7], 21)
    dense = c["x"].toarray().astype(np.float32).astype(np.float64)  # float32 numbers: the same matrix in both types
    w = dense.shape[1]
    assert w % 64 and w % 4
    sigma, a = 0.1, 0.2
    want, want_fraction, _ = so.cnv_states(dense, c["chr_pos"], amplitude=a, sigma=sigma)
    want_q = np.asarray(so.rowsq(dense))
    h, stay, sw = so.scalars(sigma, 1e-3)
    bounds = chromosome_bounds(c["chr_pos"], w)
    tdtype = getattr(torch, dtype)
    plain = _engine.DeviceMatrix(dense=torch.from_numpy(dense).cuda().to(tdtype))
    results = []
    for dm in [plain] + [_padded(dense, pad, tdtype) for pad in PADS]:
        q, flag = _engine.states_rowsq(dm)
        states, count = _engine.states_viterbi(dm, bounds, amplitude=a, h=h, stay=stay, sw=sw)
        assert int(flag.item()) == 0
        results.append((q.cpu().numpy(), states.cpu().numpy(), count.cpu().numpy()))
    for (q, states, count), ld in zip(results, (w,) + tuple(w + p for p in PADS)):
        assert q.tobytes() == results[0][0].tobytes() and q.tobytes() == want_q.tobytes(), ld
        assert states.tobytes() == results[0][1].tobytes() and states.tobytes() == want.tobytes(), ld
        assert np.array_equal(count, (want != 0).sum(axis=1)), ld
        assert np.array_equal(count / float(w), want_fraction), ld
    assert (want != 0).any()


# ---- B: chr_start layouts that the wrapper refuses and the C ABI documents ------------------------------------------------------
@pytest.mark.parametrize("layout", ["empty_chromosome", "uncovered_ends"])
@pytest.mark.parametrize("kind", ["csr", "dense"])
def test_chr_start_with_an_empty_chromosome_and_uncovered_windows(layout, kind):
    import torch

    from infercnvpy_amd import _engine

    c = so.planted(9, [10, 7, 13], 19, keep=0.5)
    sigma, a = 0.1, 0.2
    dense = c["x"].toarray()
    w = dense.shape[1]
    dense[:, :3], dense[:, w - 2:] = 3 * a, -3 * a  # a chain that covered these windows would call them
    x = sp.csr_matrix(dense)
    bounds = [0, 10, 10, 17, w] if layout == "empty_chromosome" else [3, 9, w - 2]
    want, want_fraction, _ = so.cnv_states(x, None, amplitude=a, sigma=sigma, bounds=bounds)
    h, stay, sw = so.scalars(sigma, 1e-3)
    dm = _engine.matrix_input(x, "test") if kind == "csr" else _engine.DeviceMatrix(dense=torch.from_numpy(x.toarray()).cuda())
    states, count = _engine.states_viterbi(dm, np.asarray(bounds, dtype=np.int32), amplitude=a, h=h, stay=stay, sw=sw)
    states, count = states.cpu().numpy(), count.cpu().numpy()
    assert states.tobytes() == want.tobytes()
    assert np.array_equal(count, (want != 0).sum(axis=1)) and np.array_equal(count / float(w), want_fraction)
    assert (want != 0).any()
    if layout == "uncovered_ends":
        assert not states[:, :3].any() and not states[:, w - 2:].any()
        covered = so.cnv_states(x, c["chr_pos"], amplitude=a, sigma=sigma)[0]
        assert covered[:, :3].all() and covered[:, w - 2:].all()
    else:
        assert np.array_equal(want, so.cnv_states(x, c["chr_pos"], amplitude=a, sigma=sigma)[0])


# ---- E: a finite value whose emission overflows ----------------------------------------------------------------------------------
def _inputs(x):
    import torch

    return {"csr": x, "dense": x.toarray(), "cuda": torch.from_numpy(x.toarray()).cuda()}


def test_emission_overflow_raises_and_nothing_is_launched(monkeypatch):
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    launched = []
    real = _engine.states_viterbi
    monkeypatch.setattr(_engine, "states_viterbi", lambda *a, **k: launched.append(1) or real(*a, **k))
    x, pos, kw = so.overflow_case()
    for sign in (1.0, -1.0):
        for name, xin in _inputs(sp.csr_matrix(sign * x.toarray())).items():
            ad = _adata(xin, pos)
            with pytest.raises(ValueError, match=r"sigma=0\.1 and amplitude=0\.2 overflow.*1e\+160"):
                cnv.tl.cnv_states(ad, **kw)
            assert "X_cnv_states" not in ad.obsm and "cnv_states" not in ad.uns and "cnv_states_fraction" not in ad.obs, name
    assert not launched


def test_largest_value_that_does_not_overflow_still_runs():
    import torch

    x, pos, kw = so.overflow_case()
    m = so.largest_value_that_does_not_overflow(kw["amplitude"], kw["sigma"])
    x.data[x.data == 1e160] = m
    want, want_fraction, _ = so.cnv_states(x, pos, **kw)
    for name, xin in _inputs(x).items():
        states, fraction = _run(xin, pos, **kw)
        if torch.is_tensor(states):
            states, fraction = states.cpu().numpy(), fraction.cpu().numpy()
        assert np.array_equal(states, want) and np.array_equal(fraction, want_fraction), name
    x.data[x.data == m] = float(np.nextafter(m, np.inf))
    with pytest.raises(ValueError, match="overflow"):
        _run(x, pos, **kw)


def test_packed_csr_with_an_unused_tail_is_judged_by_its_stored_entries():
    """The buffers of a PackedCsr may be longer than the stored entries; what lies behind them is not part of the
    matrix, whatever it holds."""
    import torch

    import infercnvpy_amd as cnv

    c = so.planted(20, [20, 9], 5)
    x = c["x"]
    kw = {"sigma": 0.1, "amplitude": 0.2}
    want, want_fraction, _ = so.cnv_states(x, c["chr_pos"], **kw)
    for tail in (1e160, np.nan, 0.0):
        data = torch.from_numpy(np.concatenate([x.data, np.full(7, tail)])).cuda()
        indices = torch.from_numpy(np.concatenate([x.indices.astype(np.int32), np.zeros(7, dtype=np.int32)])).cuda()
        packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), indices, data, x.shape[1])
        states, fraction = _run(packed, c["chr_pos"], **kw)
        assert np.array_equal(states.cpu().numpy(), want) and np.array_equal(fraction.cpu().numpy(), want_fraction)
    bad = x.copy()
    bad.data[3] = -1e160
    data = torch.from_numpy(np.concatenate([bad.data, np.zeros(7)])).cuda()
    packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), indices, data, x.shape[1])
    with pytest.raises(ValueError, match="overflow"):
        _run(packed, c["chr_pos"], **kw)

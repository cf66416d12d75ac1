"""The K-state HMM kernels at their limits ("limits pinned"): k_copy_states_viterbi where the second
best of rule 3 decides (switch probabilities above (K - 1) / K), every K in every value type and storage against the
oracle, dense input with a leading dimension above W and chr_start layouts that only the C ABI reaches in all three
kernels, ts_exp's cutoff among five states, levels off every lattice, and rule 4's order stated by hand.  Every
comparison is on bytes."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _copy_fit_oracle as cfo
import _copy_posterior_oracle as cpo
import _copy_states_oracle as co
import _posterior_oracle as po
import _states_oracle as so

pytestmark = pytest.mark.gpu

ALL_K = range(co.MIN_STATES, co.MAX_STATES + 1)
PADS = (1, 64)
PAD_VALUE = 1e30  # finite in float32 and float64: a kernel that reads the padding changes every result


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _host(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


def _adata(x, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _calls(x, chr_pos, **kw):
    import infercnvpy_amd as cnv

    return tuple(_host(v) for v in cnv.tl.cnv_copy_states(_adata(x, chr_pos), inplace=False, **kw))


def _posteriors(x, chr_pos, **kw):
    import infercnvpy_amd as cnv

    planes = cnv.tl.cnv_copy_posteriors(_adata(x, chr_pos), inplace=False, all_states=True, **kw)
    return np.stack([_host(v) for v in planes])


def _same_calls(got, c, what):
    states, sign, fraction = got
    for plane in (states, sign):
        assert plane.dtype == np.int8 and plane.shape == c["states"].shape, what
    print(f"{what}: {states.shape}, {int((states != c['states']).sum())} / {int((sign != c['sign']).sum())} bytes of the two "
          "planes differ from the oracle")
    assert states.tobytes() == c["states"].tobytes(), what
    assert sign.tobytes() == c["sign"].tobytes(), what
    assert fraction.dtype == np.float64 and fraction.tobytes() == c["fraction"].tobytes(), what


def _same_floats(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    differ = int((_bits(got) != _bits(want)).sum())
    print(f"{what}: {want.shape}, {differ} float64 differ from the oracle")
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), what


def _model(kw):
    """(levels, neutral, h, (stay, sw), (ps, pw)) of a case's kwargs: what the engine bindings take."""
    mu, z = co.check_levels(kw["levels"])
    h, stay, sw = co.scalars(kw["sigma"], kw["switch_prob"], len(mu))
    _, ps, pw = cpo.scalars(kw["sigma"], kw["switch_prob"], len(mu))
    return mu, z, h, (stay, sw), (ps, pw)


def _engine_run(dm, bounds, kw):
    """The three chain kernels through their bindings under the kernel's own chr_start array:
    dict(states, sign, count, neutral, planes, stats) of host arrays."""
    from infercnvpy_amd import _engine

    mu, z, h, (stay, sw), (ps, pw) = _model(kw)
    bounds = np.asarray(bounds, dtype=np.int32)
    states, sign, count = _engine.copy_states_viterbi(dm, bounds, levels=mu, neutral=z, h=h, stay=stay, sw=sw)
    neutral, planes = _engine.copy_posterior_chains(dm, bounds, levels=mu, neutral=z, h=h, ps=ps, pw=pw, all_states=True)
    alone, none = _engine.copy_posterior_chains(dm, bounds, levels=mu, neutral=z, h=h, ps=ps, pw=pw)
    stats = _engine.copy_posterior_stats(dm, bounds, levels=mu, neutral=z, h=h, ps=ps, pw=pw)
    assert none is None and tuple(planes.shape) == (len(mu),) + tuple(dm.shape)
    out = {"states": states, "sign": sign, "count": count, "neutral": neutral, "planes": planes, "stats": stats}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert alone.cpu().numpy().tobytes() == out["neutral"].tobytes() == out["planes"][z].tobytes()
    return out


def _oracle_run(x, bounds, kw):
    """What ``_engine_run`` must give, from the three oracles under ``bounds=``."""
    states, sign, _, _ = co.cnv_copy_states(x, None, bounds=bounds, **kw)
    planes, params = cpo.cnv_copy_posteriors(x, None, bounds=bounds, **kw)
    stats = cfo.stats(x, None, kw["levels"], kw["sigma"], kw["switch_prob"], bounds=bounds)
    assert np.isfinite(stats).all()
    return {"states": states, "sign": sign, "count": (states != 0).sum(axis=1).astype(np.int32),
            "neutral": planes[params["neutral"]], "planes": planes, "stats": stats}


def _same_run(got, want, what):
    for key, ref in want.items():
        differ = int((got[key] != ref).sum()) if key in ("states", "sign", "count") else int((_bits(got[key]) != _bits(ref)).sum())
        print(f"{what}, {key}: {differ} of {ref.size} values differ")
        assert got[key].dtype == ref.dtype and got[key].tobytes() == np.ascontiguousarray(ref).tobytes(), (what, key)


# ---- A: the second best of rule 3 decides ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ALL_K)
def test_switch_probability_above_k_minus_1_over_k_equals_the_oracle(k):
    """At switch_prob = 0.999 leaving costs less than staying, state a1 takes m2 / a2 and the backtrack its
    ``s == b1 ? b2 : b1``.  tests/test_copy_states_oracle.py shows that a dropped demotion, a dropped second-best branch
    and m1 for every state each change at least 8, 10 and 42 chains of every one of these cases, and none at the
    switch probabilities of the other tests."""
    for z in co.high_switch_positions(k):
        c = co.case(f"every_k_{k}_{z}_{co.HIGH_SWITCH}")
        assert c["kwargs"]["switch_prob"] == co.HIGH_SWITCH > (k - 1) / k
        _same_calls(_calls(c["x"], c["chr_pos"], **c["kwargs"]), c, f"K = {k}, z = {z}")
        low = co.case(f"every_k_{k}_{z}_0.3")  # the same matrix: the parameter reached the kernel
        assert (low["x"] != c["x"]).nnz == 0 and (low["states"] != c["states"]).sum() >= 100


# ---- B: every K in every value type and storage ----------------------------------------------------------------------------------
FORM_Z = {2: 1, 3: 0, 4: 2, 5: 4, 6: 0, 7: 3, 8: 7}  # one of the first, the middle and the last state
FORMS = ("csr_float32", "dense_float32", "dense_float64", "cuda_float32")


def _form(x, form):
    import torch

    dense = x.toarray()
    assert np.array_equal(dense, dense.astype(np.float32).astype(np.float64))  # multiples of 0.25: float32 numbers
    return {"csr_float32": lambda: x.astype(np.float32), "dense_float32": lambda: dense.astype(np.float32),
            "dense_float64": lambda: dense, "cuda_float32": lambda: torch.from_numpy(dense.astype(np.float32)).cuda()}[form]()


@functools.lru_cache(maxsize=None)
def _every_k_stats(name):
    c = cpo.case(name)
    kw = c["kwargs"]
    want = cfo.stats(c["x"], c["chr_pos"], kw["levels"], kw["sigma"], kw["switch_prob"])
    assert np.isfinite(want).all()
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", ALL_K)
def test_every_k_in_every_value_type_and_storage_equals_the_oracle(k, form):
    """``by_states`` x ``hmm_launch`` pick one of 28 instantiations per kernel; the CSR float64 ones meet the oracle in the
    every-K tests, these are the other 21 of each kernel, on the same cases and the same expected bytes."""
    import torch

    from infercnvpy_amd import _engine, _lib

    z = FORM_Z[k]
    assert z in co.high_switch_positions(k)
    for p in co.EVERY_K_SWITCH + (co.HIGH_SWITCH,):
        name = f"every_k_{k}_{z}_{p}"
        c = co.case(name)
        x = _form(c["x"], form)
        assert torch.is_tensor(x) == (form == "cuda_float32")
        _same_calls(_calls(x, c["chr_pos"], **c["kwargs"]), c, f"{name} {form}")
        if p == co.HIGH_SWITCH:
            continue
        _same_floats(_posteriors(x, c["chr_pos"], **c["kwargs"]), cpo.case(name)["planes"], f"{name} {form} planes")
        mu, zz, h, _, (ps, pw) = _model(c["kwargs"])
        dm = _engine.matrix_input(x, "test")
        assert dm.dtype == (torch.float64 if form == "dense_float64" else torch.float32)
        assert (dm.format == _lib.ICV_CSR) == (form == "csr_float32") and zz == z
        stats = _engine.copy_posterior_stats(dm, so.bounds(c["chr_pos"], c["x"].shape[1]), levels=mu, neutral=z, h=h, ps=ps,
                                             pw=pw).cpu().numpy()
        _same_floats(stats, _every_k_stats(name), f"{name} {form} statistics")


# ---- C: layouts through the engine bindings ---------------------------------------------------------------------------------------
LAYOUT_MODELS = ((2, 0), (5, 3), (8, 6))  # (K, z): the neutral state first, above the middle, next to the last
LAYOUT_STEP, LAYOUT_SIGMA = 0.3, 0.1  # so.planted shifts its segments by 6 sigma: two steps


def _layout_kwargs(k, z):
    return {"levels": [(s - z) * LAYOUT_STEP for s in range(k)], "sigma": LAYOUT_SIGMA, "switch_prob": 1e-3}


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
@pytest.mark.parametrize("k, z", LAYOUT_MODELS)
def test_padded_dense_rows_equal_the_contiguous_matrix_and_the_oracle(k, z, dtype):
    import torch

    from infercnvpy_amd import _engine

    c = so.planted(12, [33, 1, 70, 7], 21)
    dense = c["x"].toarray().astype(np.float32).astype(np.float64)  # float32 numbers: the same matrix in both types
    w = dense.shape[1]
    assert w % 64 and w % 4 and w > 64
    kw = _layout_kwargs(k, z)
    bounds = so.bounds(c["chr_pos"], w)
    want = _oracle_run(sp.csr_matrix(dense), bounds, kw)
    assert (want["states"] != 0).any()
    tdtype = getattr(torch, dtype)
    plain = _engine_run(_engine.DeviceMatrix(dense=torch.from_numpy(dense).cuda().to(tdtype)), bounds, kw)
    _same_run(plain, want, f"K = {k}, {dtype}, ld = {w}")
    for pad in PADS:
        got = _engine_run(_padded(dense, pad, tdtype), bounds, kw)
        _same_run(got, plain, f"K = {k}, {dtype}, ld = {w + pad} against the contiguous run")
        _same_run(got, want, f"K = {k}, {dtype}, ld = {w + pad}")


def _layout_case(k, z):
    """12 rows over (10, 7, 13) windows; the first three and the last two windows hold values three steps from 0, on the
    side where the model has states: a chain that covered them would call them."""
    c = so.planted(12, [10, 7, 13], 19, keep=0.5)
    dense = c["x"].toarray()
    w = dense.shape[1]
    assert w % 4 and w % 64
    dense[:, :3] = (3 if z < k - 1 else -3) * LAYOUT_STEP
    dense[:, w - 2:] = (-3 if z > 0 else 3) * LAYOUT_STEP
    return sp.csr_matrix(dense), c["chr_pos"], w


def _layout_matrix(x, kind):
    import torch

    from infercnvpy_amd import _engine

    return _engine.matrix_input(x, "test") if kind == "csr" else _engine.DeviceMatrix(dense=torch.from_numpy(x.toarray()).cuda())


@pytest.mark.parametrize("kind", ["csr", "dense"])
@pytest.mark.parametrize("k, z", LAYOUT_MODELS)
def test_chr_start_with_an_empty_chromosome(k, z, kind):
    x, chr_pos, w = _layout_case(k, z)
    kw = _layout_kwargs(k, z)
    dm = _layout_matrix(x, kind)
    whole = _engine_run(dm, so.bounds(chr_pos, w), kw)
    got = _engine_run(dm, [0, 10, 10, 17, w], kw)
    _same_run(got, whole, f"K = {k}, {kind}: [0, 10, 10, 17, W] against [0, 10, 17, W]")
    _same_run(got, _oracle_run(x, [0, 10, 10, 17, w], kw), f"K = {k}, {kind}: [0, 10, 10, 17, W]")
    assert (got["states"] != 0).any()


@pytest.mark.parametrize("kind", ["csr", "dense"])
@pytest.mark.parametrize("k, z", LAYOUT_MODELS)
def test_chr_start_with_windows_that_no_chromosome_covers(k, z, kind):
    x, chr_pos, w = _layout_case(k, z)
    kw = _layout_kwargs(k, z)
    bounds = [3, 9, w - 2]
    want = _oracle_run(x, bounds, kw)
    got = _engine_run(_layout_matrix(x, kind), bounds, kw)
    covered = co.cnv_copy_states(x, chr_pos, **kw)[0]
    assert covered[:, :3].all() and covered[:, w - 2:].all()  # (a chain over these windows calls them)
    for cols in (slice(0, 3), slice(w - 2, w)):
        assert not got["states"][:, cols].any() and not got["sign"][:, cols].any()
        for s in range(k):  # 1.0 in plane z, +0.0 in every other
            assert (_bits(got["planes"][s][:, cols]) == _bits(np.float64(1.0 if s == z else 0.0))).all(), s
        assert (_bits(got["neutral"][:, cols]) == _bits(np.float64(1.0))).all()
    assert np.array_equal(got["count"], (got["states"][:, 3:w - 2] != 0).sum(axis=1))
    assert (got["count"] < (covered != 0).sum(axis=1)).all() and (got["states"] != 0).any()
    _same_run(got, want, f"K = {k}, {kind}: [3, 9, W - 2]")


# ---- D: values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["csr_float64", "dense_float32"])
def test_five_level_cutoff_case_equals_the_oracle(form):
    """tests/test_copy_posterior_oracle.py shows where the case sits: in a probe window two states have b = 0.0 exactly,
    the neutral one exp_(-707), exp_(-708) or 0.0, and every plane holds exact zeros next to non-zero posteriors."""
    from infercnvpy_amd import _engine

    c = cpo.case("exp_cutoff5")
    kw = c["kwargs"]
    assert np.array_equal(c["x"].data, c["x"].data.astype(np.float32).astype(np.float64))  # every value a float32 number
    x = c["x"] if form == "csr_float64" else c["x"].toarray().astype(np.float32)
    _same_floats(_posteriors(x, c["chr_pos"], **kw), c["planes"], f"exp_cutoff5 {form} planes")
    want = cfo.stats(c["x"], c["chr_pos"], kw["levels"], kw["sigma"], kw["switch_prob"])
    assert np.isfinite(want).all()
    mu, z, h, _, (ps, pw) = _model(kw)
    stats = _engine.copy_posterior_stats(_engine.matrix_input(x, "test"), so.bounds(c["chr_pos"], c["x"].shape[1]), levels=mu,
                                         neutral=z, h=h, ps=ps, pw=pw).cpu().numpy()
    _same_floats(stats, want, f"exp_cutoff5 {form} statistics")
    probes = {(row, t) for row, t, v in c["probes"] if v == cpo.CUTOFF5_VALUES[2]}
    assert len(probes) == 2 * len(po.CUTOFF_PROBES) and all(c["planes"][z, row, t] == 0.0 for row, t in probes)


def test_levels_off_every_lattice_equal_the_oracle():
    from infercnvpy_amd import _engine

    c = co.case("unequal_levels")
    kw = c["kwargs"]
    states, sign, fraction = _calls(c["x"], c["chr_pos"], **kw)
    _same_calls((states, sign, fraction), c, "unequal_levels")
    assert len(np.unique(states)) >= 5
    planes = cpo.case("unequal_levels")["planes"]
    _same_floats(_posteriors(c["x"], c["chr_pos"], **kw), planes, "unequal_levels planes")
    want = cfo.stats(c["x"], c["chr_pos"], kw["levels"], kw["sigma"], kw["switch_prob"])
    mu, z, h, _, (ps, pw) = _model(kw)
    stats = _engine.copy_posterior_stats(_engine.matrix_input(c["x"], "test"), so.bounds(c["chr_pos"], c["x"].shape[1]),
                                         levels=mu, neutral=z, h=h, ps=ps, pw=pw).cpu().numpy()
    _same_floats(stats, want, "unequal_levels statistics")


# ---- E: rule 4 by hand ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", range(co.END_RULE_STATES))
def test_end_rule_hand_table(z):
    """Seven one-window chromosomes, each half-way between two adjacent levels of eight: the state nearer to z wins, and z
    wins against both its neighbours.  ``want`` is written by hand in the builder."""
    c = co.end_rule(z)
    states, sign, fraction = _calls(c["x"], c["chr_pos"], **c["kwargs"])
    print(f"z = {z}: {states[0].tolist()}, by hand {c['want'][0].tolist()}")
    assert states.dtype == np.int8 and states.tobytes() == c["want"].tobytes()
    assert sign.tobytes() == np.sign(c["want"]).tobytes()
    assert fraction.tolist() == [int((c["want"] != 0).sum()) / 7.0]

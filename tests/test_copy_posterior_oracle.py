"""The oracle of tl.cnv_copy_posteriors and tl.cnv_copy_states_filter (tests/_copy_posterior_oracle.py)
against the three-state oracle, against an independent log-space forward-backward and on the planted multi-level chain;
the header, the library and the argument validation of the C ABI and of the public functions -- none of it needs a
GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _copy_posterior_oracle as cpo
import _copy_states_oracle as co
import _posterior_oracle as po
import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_K = range(cpo.MIN_STATES, cpo.MAX_STATES + 1)
# The largest |oracle - log-space forward-backward| over every_k(k, z, p), all z and both EVERY_K_SWITCH, measured on the
# CPU per K = 2 .. 8: 1.8e-15, 3.6e-15, 7.4e-15, 9.0e-15, 1.0e-14, 1.4e-14, 1.1e-14.  The bound is four times the largest.
LOG_SPACE_MEASURED = 1.3877787807814457e-14
LOG_SPACE_BOUND = 4 * LOG_SPACE_MEASURED
ULP = 2.0 ** -52
# the cases of tests/test_gpu_copy_posteriors.py on which the deviations are looked for
PARITY_SAMPLE = ("every_k_6_2_0.001", "every_k_6_2_0.3", "every_k_3_1_0.3", "every_k_2_0_0.3", "planted_levels_2",
                 "chromosomes_65")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- the rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", po.CASE_NAMES)
def test_three_levels_are_the_three_state_oracle_bit_for_bit(name):
    c = po.case(name)
    a, sigma, p = c["params"]["amplitude"], c["params"]["sigma"], c["params"]["switch_prob"]
    planes, params = cpo.cnv_copy_posteriors(c["x"], c["chr_pos"], levels=(-a, 0.0, a), sigma=sigma, switch_prob=p)
    assert params == {"levels": [-a, 0.0, a], "neutral": 1, "sigma": sigma, "switch_prob": p}
    for plane, key in zip(planes, ("loss", "neutral", "gain")):
        differ = int((_bits(plane) != _bits(c[key])).sum())
        print(f"{name}: {differ} of {plane.size} float64 of {key} differ from the three-state oracle")
        assert differ == 0


@pytest.mark.parametrize("k", ALL_K)
def test_oracle_agrees_with_a_log_space_forward_backward(k):
    worst = 0.0
    for z in range(k):
        for p in co.EVERY_K_SWITCH:
            c = cpo.case(f"every_k_{k}_{z}_{p}")
            mu, zz = co.check_levels(c["kwargs"]["levels"])
            assert zz == z and c["planes"].shape[0] == k
            dense = c["x"].toarray()
            edges = so.bounds(c["chr_pos"], dense.shape[1])
            for s0, s1 in zip(edges[:-1], edges[1:]):
                ref = cpo.log_space_posteriors(dense[:, s0:s1], mu, c["kwargs"]["sigma"], p)
                worst = max(worst, float(np.abs(ref - c["planes"][:, :, s0:s1]).max()))
    print(f"K = {k}: the largest |oracle - log space| is {worst:.3e} (bound {LOG_SPACE_BOUND:.3e})")
    assert worst <= LOG_SPACE_BOUND


def test_planes_sum_to_one_within_four_ulp():
    """Measured on the planted case: 2.2e-16, one ulp."""
    names = [f"planted_levels_{cpo.CHAIN_SEED}"] + [f"every_k_{k}_{k // 2}_0.3" for k in ALL_K] + list(cpo.SHAPE_NAMES)
    for name in names:
        planes = cpo.case(name)["planes"]
        worst = float(np.abs(planes.sum(axis=0) - 1.0).max())
        print(f"{name}: the planes sum to 1 within {worst:.3e}")
        assert worst <= 4 * ULP and planes.min() >= 0.0 and planes.max() <= 1.0


@pytest.mark.parametrize("deviation", cpo.DEVIATIONS)
def test_every_deviation_from_the_written_sums_is_visible_on_the_parity_cases(deviation):
    """The float64 that differ from the contract's, measured on the CPU over PARITY_SAMPLE (of 5 040, 5 040, 2 304,
    1 488, 18 720 and 10 332): ok_form 2 279, 2 194, 825, 239, 10 256, 3 499; descending 2 844, 2 839, 941, 0, 11 437,
    3 399 (two terms commute); fma 2 122, 1 794, 619, 341, 10 297, 2 553.  A kernel that forms pred or v in the
    deviation's way cannot equal the contract's bytes on these cases."""
    total = 0
    for name in PARITY_SAMPLE:
        c = cpo.case(name)
        got, _ = cpo.cnv_copy_posteriors(c["x"], c["chr_pos"], deviation=deviation, **c["kwargs"])
        differ = int((_bits(got) != _bits(c["planes"])).sum())
        print(f"{deviation}: {differ} of {got.size} float64 of {name} differ from the contract's")
        assert np.abs(got - c["planes"]).max() < 1e-12  # (the same model, another rounding)
        total += differ
        if name.startswith("every_k_6") or name == "planted_levels_2":
            assert differ >= 1, name
    assert total >= 1


def test_uncovered_windows_zero_matrix_and_default_levels():
    c = so.planted(12, [20, 1, 9], 4)
    kw = {"levels": (-0.2, 0.0, 0.2, 0.4), "sigma": 0.1}
    part, params = cpo.cnv_copy_posteriors(c["x"], None, bounds=[3, 9, 9, 28], **kw)
    assert params["neutral"] == 1 and part.shape == (4, 12, 30)
    for cols in (slice(0, 3), slice(28, 30)):
        assert (part[1][:, cols] == 1.0).all() and not part[[0, 2, 3]][:, :, cols].any()
    alone, _ = cpo.cnv_copy_posteriors(c["x"][:, 3:9], {"c": 0}, **kw)
    assert np.array_equal(_bits(part[:, :, 3:9]), _bits(alone))
    zero, params = cpo.cnv_copy_posteriors(sp.csr_matrix((3, 30)), c["chr_pos"])
    assert params["sigma"] == 0.0 and zero.shape == (6, 3, 30) and (zero[2] == 1.0).all() and zero.sum() == 90.0
    planes, params = cpo.cnv_copy_posteriors(c["x"], c["chr_pos"])
    sigma = so.default_sigma(c["x"])
    assert params == {"levels": [float(k) * (2.0 * sigma) for k in co.DEFAULT_STEPS], "neutral": 2, "sigma": sigma,
                      "switch_prob": 1e-3}
    assert cpo.plane_names(6, 2) == ["loss2", "loss1", "neutral", "gain1", "gain2", "gain3"]
    assert cpo.plane_names(2, 0) == ["neutral", "gain1"] and cpo.plane_names(3, 2) == ["loss2", "loss1", "neutral"]
    x, pos, okw = so.overflow_case()
    with pytest.raises(ValueError, match="overflow"):
        cpo.cnv_copy_posteriors(x, pos, levels=(-0.2, 0.0, 0.2, 0.4), sigma=okw["sigma"])


def test_five_level_cutoff_case_sits_on_the_cutoff_of_the_written_exponential():
    """What the K = 5 case adds to the three-level ``exp_cutoff``: in one window two states lie beyond the cutoff (b
    exactly 0.0), one lies on or next to it and one is about 1e-153."""
    from _tsne_oracle import exp_

    assert float(exp_(np.float64(-708.0))) > 0.0 and float(exp_(np.nextafter(np.float64(-708.0), -np.inf))) == 0.0
    c = cpo.case("exp_cutoff5")
    mu, z = co.check_levels(c["kwargs"]["levels"])
    h = cpo.scalars(c["kwargs"]["sigma"], c["kwargs"]["switch_prob"], 5)[0]
    assert h == 8.0 and z == 2 and c["planes"].shape == (5,) + c["x"].shape
    for v, gap in zip(cpo.CUTOFF5_VALUES, cpo.CUTOFF5_GAPS):
        assert np.float32(v) == v
        for sign in (1.0, -1.0):
            e = co.emissions(sign * v, mu, h)
            assert e[z] - max(e) == gap and max(e) == (e[4] if sign > 0 else e[0])
            b = [float(u[0]) for u in cpo.emissions(np.array([sign * v]), mu, h)]
            b = b if sign > 0 else b[::-1]
            assert b[0] == b[1] == 0.0 and (b[2] > 0.0) == (gap >= -708.0) and 0.0 < b[3] < 1e-150 and b[4] == 1.0
    planes = c["planes"]
    assert np.isfinite(planes).all() and (planes >= 0.0).all() and (planes <= 1.0).all()
    zeros = [int(((p == 0.0).any(axis=1) & (p != 0.0).any(axis=1)).sum()) for p in planes]
    print(f"rows of each plane with an exact 0.0 next to a non-zero posterior: {zeros}")
    assert all(n >= 1 for n in zeros)
    seen = {v: [] for v in cpo.CUTOFF5_VALUES}
    for row, t, v in c["probes"]:
        seen[v].append(float(planes[z, row, t]))
    print({v: (min(p), max(p)) for v, p in seen.items()})
    assert all(len(p) == 2 * len(po.CUTOFF_PROBES) for p in seen.values())
    assert all(0.0 < p < 1e-300 for p in seen[44.6875]) and all(0.0 < p < 1e-300 for p in seen[44.75])
    assert all(p == 0.0 for p in seen[44.8125])  # the -708 and the -709 probes differ in the neutral plane


# ---- the chain on the planted case -------------------------------------------------------------------------------------------
def test_chain_constants_on_the_planted_case():
    c = cpo.chain_case()
    truth, states, filtered = c["truth"], c["states"], c["filtered"]
    gone = [(i, s, e, m) for i, s, e, m in c["means"] if m > cpo.CHAIN_MAX_P_NORMAL]
    right = [m for i, s, e, m in c["means"] if np.array_equal(states[i, s:e], truth[i, s:e])]
    print(f"removed runs (row, start, end, mean): {gone}; the largest mean of a run whose call is right: {max(right)!r}; "
          f"wrong calls {int((states != truth).sum())} -> {int((filtered != truth).sum())}")
    assert int(c["removed"].sum()) == len(gone) == 2
    for (i, s, e, m), want in zip(sorted(gone, key=lambda r: -r[3]), cpo.CHAIN_REMOVED_MEANS):
        assert e - s == 1 and truth[i, s] == 0 and states[i, s] != 0 and not filtered[i, s]  # a one-window false call
        assert abs(m - want) < 5e-4
    assert abs(max(right) - cpo.CHAIN_LARGEST_RIGHT_MEAN) < 5e-4 and max(right) <= cpo.CHAIN_MAX_P_NORMAL
    assert int((states != truth).sum()) == cpo.CHAIN_WRONG_BEFORE
    assert int((filtered != truth).sum()) == cpo.CHAIN_WRONG_AFTER
    assert np.array_equal(c["sign"], np.sign(filtered)) and np.array_equal(c["fraction"], (filtered != 0).sum(axis=1) / 130.0)


# ---- the filter --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cpo.crafted_filter_cases()))
def test_crafted_filter_cases(name):
    c = cpo.crafted_filter_cases()[name]
    out, sign, fraction, removed, means = cpo.copy_states_filter(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])
    assert np.array_equal(out, c["want"]) and out.dtype == np.int8
    assert np.array_equal(sign, np.sign(c["want"])) and sign.dtype == np.int8
    assert int(removed.sum()) == len([m for m in means if m[3] > c["max_p_normal"]])


def test_two_levels_get_separate_verdicts_and_levels_beyond_seven_are_refused():
    c = cpo.crafted_filter_cases()["two_levels_of_one_sign_are_two_runs"]
    *_, means = cpo.copy_states_filter(c["states"], c["p"], c["chr_pos"], 0.5)
    assert [(s, e) for _, s, e, _ in means] == [(0, 2), (2, 4)]
    for level in (8, -8):
        states = np.array([[0, level, 0]], dtype=np.int8)
        with pytest.raises(ValueError, match=r"outside \[-7, 7\]"):
            cpo.copy_states_filter(states, np.zeros((1, 3)), {"a": 0})
    with pytest.raises(ValueError, match="posterior"):
        cpo.copy_states_filter(np.array([[0, 1, 0]], dtype=np.int8), np.array([[0.0, np.nan, 0.0]]), {"a": 0})


def test_filter_on_three_state_calls_is_the_three_state_filter():
    states, p = po.random_calls(30, [40, 1, 70, 19], 5)
    pos = so.chr_pos_of([40, 1, 70, 19])
    want, want_fraction, want_removed = po.states_filter(states, p, pos, 0.5)
    out, sign, fraction, removed, _ = cpo.copy_states_filter(states, p, pos, 0.5)
    assert np.array_equal(out, want) and np.array_equal(sign, want) and np.array_equal(fraction, want_fraction)
    assert np.array_equal(removed, want_removed) and removed.sum() > 10
    both = cpo.copy_states_filter(cpo.doubled({"states": states})["states"], p, pos, 0.5)
    assert np.array_equal(both[0], 2 * want) and np.array_equal(both[1], want) and np.array_equal(both[3], want_removed)
    case = po.sweep_cases("behind_other_sign")[0]
    alt = cpo.alternating(case)
    assert set(np.unique(np.abs(alt["states"]))) == {0, 1, 2}
    for i, (s, e) in enumerate(case["main"]):
        assert np.array_equal(alt["states"][i, s:e], case["states"][i, s:e])
    assert np.array_equal(np.sign(alt["states"]), np.sign(case["states"]))


# ---- the header, the library and the C ABI -----------------------------------------------------------------------------------
def test_caps_agree_and_symbols_are_exported():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    budget = int(re.search(r"#define\s+ICV_COPY_POSTERIOR_LDS_BYTES\s+(\d+)", header).group(1))
    macro = re.search(r"#define\s+ICV_COPY_POSTERIOR_MAX_WINDOWS\(k\)\s+(.+)", header).group(1).strip()
    assert macro == "(ICV_COPY_POSTERIOR_LDS_BYTES / (8 * ((k) + 1)))"
    source = open(os.path.join(ROOT, "infercnvpy_amd", "csrc", "icv_copy_posterior.hpp")).read()
    assert f"kCpLdsBytes = {budget};" in source and "return kCpLdsBytes / (8 * (k + 1));" in source
    assert budget == _lib.ICV_COPY_POSTERIOR_LDS_BYTES == cpo.LDS_BYTES == 163840
    caps = []
    for k in ALL_K:
        cap = budget // (8 * (k + 1))
        assert cap == _lib.ICV_COPY_POSTERIOR_MAX_WINDOWS(k) == cpo.max_windows(k)
        assert 8 * (k + 1) * cap <= 163840 < 8 * (k + 1) * (cap + 1)
        caps.append(cap)
    assert caps == [6826, 5120, 4096, 3413, 2925, 2560, 2275]
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_copy_posterior_chains", "icv_copy_states_filter"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
    assert callable(_engine.copy_posterior_chains) and callable(_engine.copy_states_filter)
    for name in ("cnv_copy_posteriors", "cnv_copy_states_filter"):
        assert name in cnv.tl.__all__ and callable(getattr(cnv.tl, name))


def test_posterior_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    m = _lib.Matrix()
    m.format, m.dtype, m.n_rows, m.values = _lib.ICV_DENSE, _lib.ICV_F64, 0, 8
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first

    def call(levels, neutral, h=8.0, ps=0.999, pw=None, n_chr=2, n_levels=None, outputs=(one, one)):
        mu = (ctypes.c_double * len(levels))(*levels)
        k = len(levels) if n_levels is None else n_levels
        rc = lib.icv_copy_posterior_chains(ctypes.byref(m), one, n_chr, mu, k, neutral, h, ps,
                                           0.001 / max(k - 1, 1) if pw is None else pw, *outputs, None)
        return rc, lib.icv_last_error().decode()

    for k in ALL_K:
        for z in (0, k - 1):
            cap = cpo.max_windows(k)
            m.n_cols = m.ld = cap + 1
            rc, msg = call(co.every_k_levels(k, z), z)
            assert rc == _lib.ICV_ERR_INVALID and msg.startswith("copy_posterior_chains: ")
            assert f"[1, {cap}]" in msg and f"K = {k}" in msg and f"{8 * (k + 1)} bytes" in msg, msg
            m.n_cols = m.ld = cap
            assert call(co.every_k_levels(k, z), z)[0] == _lib.ICV_OK  # no rows: nothing runs
    good = [-0.5, 0.0, 0.5, 1.0]
    m.n_cols = m.ld = 0
    assert call(good, 1)[0] == _lib.ICV_ERR_INVALID
    m.n_cols = m.ld = 10
    assert call(good, 1)[0] == _lib.ICV_OK
    assert call(good, 1, outputs=(one, None))[0] == _lib.ICV_OK  # the planes are optional
    for n_chr in (0, 11):
        assert call(good, 1, n_chr=n_chr)[0] == _lib.ICV_ERR_INVALID
    inf, nan = float("inf"), float("nan")
    bad = [  # every bad model of icv_copy_states_viterbi's test
        (dict(levels=[0.0], neutral=0), "n_levels"),
        (dict(levels=[0.0] + [0.1 * k for k in range(1, 9)], neutral=0), "n_levels"),
        (dict(levels=good, neutral=1, n_levels=0), "n_levels"),
        (dict(levels=good, neutral=-1), "neutral"),
        (dict(levels=good, neutral=4), "neutral"),
        (dict(levels=good, neutral=2), "levels[neutral]"),
        (dict(levels=[-0.5, 0.0, inf], neutral=1), "finite"),
        (dict(levels=[-0.5, 0.0, nan], neutral=1), "finite"),
        (dict(levels=[-inf, 0.0, 0.5], neutral=1), "finite"),
        (dict(levels=[-0.5, 0.0, 0.0, 0.5], neutral=1), "ascend"),
        (dict(levels=[0.5, 0.0, -0.5], neutral=1), "ascend"),
        (dict(levels=good, neutral=1, h=0.0), "h must"),
        (dict(levels=good, neutral=1, h=inf), "h must"),
        (dict(levels=good, neutral=1, h=-1.0), "h must"),
        (dict(levels=good, neutral=1, h=nan), "h must"),
        # this entry's own scalars
        (dict(levels=good, neutral=1, ps=0.0), "ps"),
        (dict(levels=good, neutral=1, ps=1.0), "ps"),
        (dict(levels=good, neutral=1, ps=-0.5), "ps"),
        (dict(levels=good, neutral=1, ps=nan), "ps"),
        (dict(levels=good, neutral=1, pw=0.0), "pw"),
        (dict(levels=good, neutral=1, pw=5e-324), "pw"),  # subnormal
        (dict(levels=good, neutral=1, pw=-0.1), "pw"),
        (dict(levels=good, neutral=1, pw=1.0), "pw"),
        (dict(levels=good, neutral=1, pw=inf), "pw"),
        (dict(levels=good, neutral=1, pw=nan), "pw"),
    ]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == _lib.ICV_ERR_INVALID and msg.startswith("copy_posterior_chains: ") and word in msg, (kw, msg)
    assert call(good, 1, outputs=(None, one))[0] == _lib.ICV_ERR_INVALID  # P(neutral) is always written
    mu = (ctypes.c_double * 4)(*good)
    args = (4, 1, 8.0, 0.999, 0.001 / 3, one, one, None)
    assert lib.icv_copy_posterior_chains(ctypes.byref(m), one, 2, None, *args) == _lib.ICV_ERR_INVALID
    assert lib.icv_copy_posterior_chains(None, one, 2, mu, *args) == _lib.ICV_ERR_INVALID
    assert lib.icv_copy_posterior_chains(ctypes.byref(m), None, 2, mu, *args) == _lib.ICV_ERR_INVALID
    assert call([-0.5, -0.0, 0.5], 1)[0] == _lib.ICV_OK  # -0.0 is a zero


def test_filter_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced

    def call(n_rows=4, n_cols=10, n_chr=2, thr=0.5, ptrs=(one,) * 8):
        states, p, chr_start, filtered, sign, count, removed, bad = ptrs
        rc = lib.icv_copy_states_filter(states, p, n_rows, n_cols, chr_start, n_chr, thr, filtered, sign, count, removed,
                                        bad, None)
        return rc, lib.icv_last_error().decode()

    for k in range(8):
        rc, msg = call(ptrs=tuple(None if i == k else one for i in range(8)))
        assert rc == _lib.ICV_ERR_INVALID and msg == "bad copy_states_filter arguments", k
    for kw in ({"n_rows": -1}, {"n_cols": 0}, {"n_chr": 0}, {"n_chr": 11}, {"thr": -0.1}, {"thr": 1.5},
               {"thr": float("nan")}):
        assert call(**kw)[0] == _lib.ICV_ERR_INVALID, kw
    rc, msg = call(n_cols=_lib.ICV_FILTER_MAX_WINDOWS + 1)
    assert rc == _lib.ICV_ERR_UNSUPPORTED and msg.startswith("copy_states_filter: ") and "int64" in msg


# ---- the public functions' argument validation -------------------------------------------------------------------------------
def _adata(n=4, w=10, chr_pos=None, x=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


@pytest.fixture
def no_device(monkeypatch):
    """Every way from the functions to the device raises AssertionError: the argument errors must come first."""
    from infercnvpy_amd import _engine

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were refused")

    for name in ("matrix_input", "dense_input", "states_rowsq", "states_absmax", "copy_posterior_chains",
                 "copy_states_filter", "_torch"):
        monkeypatch.setattr(_engine, name, touched)


def test_missing_keys_raise_keyerror_with_the_functions_name(no_device):
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(KeyError, match=r"tl\.cnv_copy_posteriors: X_other not found in adata\.obsm"):
        cnv.tl.cnv_copy_posteriors(ad, use_rep="other")
    with pytest.raises(KeyError, match=r"tl\.cnv_copy_states_filter: X_cnv_copy_states not found"):
        cnv.tl.cnv_copy_states_filter(ad)
    ad.obsm["X_cnv_copy_states"] = np.zeros((4, 10), dtype=np.int8)
    with pytest.raises(KeyError, match=r"tl\.cnv_copy_states_filter: X_cnv_copy_posterior_neutral not found"):
        cnv.tl.cnv_copy_states_filter(ad)
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match=r"tl\.cnv_copy_posteriors: chr_pos not found in adata\.uns\['cnv'\]"):
        cnv.tl.cnv_copy_posteriors(ad)


@pytest.mark.parametrize("k", ALL_K)
def test_window_cap_depends_on_k_and_the_message_names_it(no_device, k):
    import infercnvpy_amd as cnv

    cap = cpo.max_windows(k)
    ad = _adata(n=1, x=sp.csr_matrix((1, cap + 1)), chr_pos={"chr1": 0})
    with pytest.raises(ValueError) as err:
        cnv.tl.cnv_copy_posteriors(ad, levels=co.every_k_levels(k, k // 2), sigma=0.25)
    assert str(err.value) == (f"tl.cnv_copy_posteriors: {cap + 1} windows; the kernel keeps a cell's windows and the "
                              f"forward variables of K = {k} states in LDS and takes at most {cap}")
    if k == 6:  # the default levels are six, and so are stored ones
        with pytest.raises(ValueError, match=f"K = 6 states in LDS and takes at most {cap}"):
            cnv.tl.cnv_copy_posteriors(ad)
        ad.uns["cnv_copy_states"] = {"params": {"levels": [-0.5, 0.0, 0.5], "neutral": 1, "sigma": 0.25,
                                                "switch_prob": 1e-3}}
        with pytest.raises(ValueError, match="K = 3 states in LDS and takes at most 5120"):
            cnv.tl.cnv_copy_posteriors(_adata_with(ad, sp.csr_matrix((1, 5121))))


def _adata_with(ad, x):
    out = _adata(n=x.shape[0], x=x, chr_pos={"chr1": 0})
    out.uns["cnv_copy_states"] = ad.uns["cnv_copy_states"]
    return out


@pytest.mark.parametrize("kw, match", [
    ({"levels": (-0.3, 0.0, 0.3), "amplitude": 0.3}, "levels and amplitude"),
    ({"levels": (0.0,)}, "1 states"),
    ({"levels": [0.1 * k for k in range(9)]}, "9 states"),
    ({"levels": (-0.3, 0.0, float("inf"))}, "finite"),
    ({"levels": (-0.3, 0.0, 0.3, 0.3)}, "ascend"),
    ({"levels": (-0.3, 0.1, 0.3)}, "exactly one 0.0"),
    ({"levels": "abc"}, "sequence of numbers"),
    ({"amplitude": 0.0}, "amplitude"), ({"amplitude": float("nan")}, "amplitude"), ({"sigma": 0.0}, "sigma"),
    ({"sigma": float("inf")}, "sigma"), ({"switch_prob": 0.0}, "switch_prob"), ({"switch_prob": 1.0}, "switch_prob"),
    ({"switch_prob": float("nan")}, "switch_prob"),
    ({"switch_prob": 1e-307}, "too close to 0 or 1"),  # p / 2 is a normal float64 and p / 5 is not
    ({"switch_prob": 1e-17, "sigma": 0.1}, "too close to 0 or 1"),  # 1 - p == 1
])
def test_bad_parameters_raise_valueerror_before_the_device(no_device, kw, match):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=match) as err:
        cnv.tl.cnv_copy_posteriors(_adata(), **kw)
    assert str(err.value).startswith("tl.cnv_copy_posteriors: ")


@pytest.mark.parametrize("kw, match", [({"max_p_normal": -0.1}, "max_p_normal"), ({"max_p_normal": 1.5}, "max_p_normal"),
                                       ({"max_p_normal": float("nan")}, "max_p_normal"),
                                       ({"max_p_normal": "high"}, "max_p_normal"), ({"max_p_normal": True}, "max_p_normal")])
def test_filter_bad_threshold_raises_before_the_device(no_device, kw, match):
    import infercnvpy_amd as cnv

    ad = _adata()
    ad.obsm["X_cnv_copy_states"] = np.zeros((4, 10), dtype=np.int8)
    ad.obsm["X_cnv_copy_posterior_neutral"] = np.ones((4, 10))
    with pytest.raises(ValueError, match=match) as err:
        cnv.tl.cnv_copy_states_filter(ad, **kw)
    assert str(err.value).startswith("tl.cnv_copy_states_filter: ")


def test_filter_refuses_wrong_shapes_and_dtypes_before_the_device(no_device):
    import infercnvpy_amd as cnv

    ad = _adata()
    ad.obsm["X_cnv_copy_posterior_neutral"] = np.ones((4, 10))
    ad.obsm["X_cnv_copy_states"] = np.zeros((4, 10), dtype=np.int16)
    with pytest.raises(ValueError, match="must be int8"):
        cnv.tl.cnv_copy_states_filter(ad)
    ad.obsm["X_cnv_copy_states"] = np.zeros((4, 9), dtype=np.int8)
    with pytest.raises(ValueError, match="has shape"):
        cnv.tl.cnv_copy_states_filter(ad)
    ad.obsm["X_cnv_copy_states"] = np.zeros((4, 10), dtype=np.int8)
    ad.obsm["X_cnv_copy_posterior_neutral"] = np.ones((4, 10), dtype=np.float32)
    with pytest.raises(ValueError, match="must be float64"):
        cnv.tl.cnv_copy_states_filter(ad)

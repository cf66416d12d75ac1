"""The oracle of tl.cnv_copy_states_fit (tests/_copy_fit_oracle.py) against the posterior oracle, the
three-state fit and the properties of expectation-maximisation, the planted case that is the reason for its start values,
and everything of the function that needs no GPU: the C ABI, the export and the argument errors."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _copy_fit_oracle as cfo
import _copy_posterior_oracle as cpo
import _copy_states_oracle as co
import _fit_oracle as fo
import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY_K = tuple(f"every_k_{k}_{z}_{p}" for k, z in ((2, 0), (3, 1), (5, 2), (8, 3)) for p in co.EVERY_K_SWITCH)
STAT_CASES = tuple(f"planted_levels_{s}" for s in range(5)) + cpo.SHAPE_NAMES + EVERY_K

# N_s and M_s against the sums of the gamma planes of _copy_posterior_oracle: the two add the same terms in another order
# (numpy's pairwise sum over the whole row there, one chain per chromosome here).  Measured over STAT_CASES: the largest
# |N_s - sum_t gamma| / W is 5.1e-16, the largest |M_s - sum_t gamma x| / sum_t |x| is 4.0e-16 and the largest
# |sum_s N_s - W| / W is 5.1e-16; the bound is 4 x the largest.
STAT_REL = 4 * 5.1e-16
# The trajectory with steps (-1, 0, 1) against _fit_oracle from the same start values: the E-steps are the same
# operations, the M-steps form the same quantities from other sums (N_0 + N_2 here, gamma_0 + gamma_2 per window there).
# Measured on planted_levels seeds 0 and 2, both fits: the largest relative difference of a parameter anywhere in the
# history is 3.8e-15 (seed 0, all three names, 15 iterations); the bound is 4 x that.
TRAJECTORY_REL = 4 * 3.8e-15

def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


@functools.lru_cache(maxsize=None)
def _planted_fit(seed, fit=("amplitude", "sigma")):
    c = co.planted_levels(seed)
    return c, cfo.cnv_copy_states_fit(c["x"], c["chr_pos"], fit=fit)


def _levels(r, h):
    return cfo.levels_of(r["steps"], h["amplitude"])


# ---- statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STAT_CASES)
def test_state_masses_and_moments_are_what_the_posteriors_say(name):
    c = cpo.case(name)
    par = c["params"]
    k = len(par["levels"])
    x = so.canonical(c["x"])
    dense = x.toarray()
    w = dense.shape[1]
    got = cfo.stats(x, c["chr_pos"], par["levels"], par["sigma"], par["switch_prob"])
    assert got.shape == (dense.shape[0], 2 * k + 1) and np.isfinite(got).all()
    gamma = c["planes"]  # K x n x W
    rel_n = float(np.abs(got[:, :k] - gamma.sum(axis=2).T).max()) / w
    scale = np.abs(dense).sum(axis=1, keepdims=True)
    rel_m = float((np.abs(got[:, k:2 * k] - (gamma * dense[None]).sum(axis=2).T) / np.maximum(scale, 1e-300)).max())
    rel_w = float(np.abs(got[:, :k].sum(axis=1) - w).max()) / w  # every window is covered
    print(f"{name}: N {rel_n:.3g}, M {rel_m:.3g}, windows {rel_w:.3g}")
    assert rel_n <= STAT_REL and rel_m <= STAT_REL and rel_w <= STAT_REL
    n_steps = cfo._n_steps(c["chr_pos"], 1, w)
    assert (got[:, 2 * k] >= 0.0).all() and (got[:, 2 * k] <= n_steps * (1 + 1e-12)).all()


@pytest.mark.parametrize("seed", [0, 2])
def test_stay_mass_is_the_bytes_of_the_three_state_oracle(seed):
    c = co.planted_levels(seed)
    for a, sigma, p in ((0.3, 0.1, 1e-3), (0.23, 0.17, 0.3)):
        got = cfo.stats(c["x"], c["chr_pos"], [-a, 0.0, a], sigma, p)
        want = fo.stats(c["x"], c["chr_pos"], a, sigma, p)
        assert np.array_equal(got[:, 6], want[:, 2]) and _bits(got[:, 6]) == _bits(want[:, 2])
    one = co.shapes()["one_window_chromosome_between_long"]
    got = cfo.stats(one["x"], one["chr_pos"], [-0.3, 0.0, 0.3], 0.1, 1e-3)
    assert np.array_equal(got[:, 6], fo.stats(one["x"], one["chr_pos"], 0.3, 0.1, 1e-3)[:, 2])


def test_stats_bounds_entry_point_adds_nothing_for_an_empty_chromosome_or_an_uncovered_window():
    c = so.planted(6, [10, 7, 13], 19)
    mu, sigma, p = [k * 0.2 for k in co.DEFAULT_STEPS], 0.1, 1e-3
    want = cfo.stats(c["x"], c["chr_pos"], mu, sigma, p)
    assert _bits(cfo.stats(c["x"], None, mu, sigma, p, bounds=[0, 10, 10, 17, 30])) == _bits(want)
    part = cfo.stats(c["x"], None, mu, sigma, p, bounds=[3, 9, 28])
    alone = cfo.stats(c["x"][:, 3:28], {"a": 0, "b": 6}, mu, sigma, p)
    assert _bits(part) == _bits(alone)


# ---- trajectory and likelihood ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [("amplitude", "sigma"), cfo.NAMES], ids=["default", "all_three"])
@pytest.mark.parametrize("seed", [0, 2])
def test_three_steps_follow_the_three_state_fit(seed, fit):
    c = co.planted_levels(seed)
    sigma = cfo.start_sigma(so.canonical(c["x"]), c["chr_pos"])
    got = cfo.cnv_copy_states_fit(c["x"], c["chr_pos"], steps=(-1, 0, 1), fit=fit)
    want = fo.cnv_states_fit(c["x"], c["chr_pos"], amplitude=2.0 * sigma, sigma=sigma, fit=fit)
    assert (got["n_iter"], got["converged"], got["fit"]) == (want["n_iter"], want["converged"], want["fit"])
    assert got["converged"] and got["n_iter"] >= 3 and len(got["history"]) == len(want["history"]) == got["n_iter"] + 1
    assert got["history"][0] == want["history"][0]
    worst = max(abs(a[key] - b[key]) / b[key] for a, b in zip(got["history"], want["history"]) for key in cfo.NAMES)
    print(f"seed {seed}, {fit}: {got['n_iter']} iterations, largest relative difference {worst:.3g}")
    assert worst <= TRAJECTORY_REL
    a = got["amplitude"]
    assert got["params"] == {"levels": [-1.0 * a, 0.0, a], "sigma": got["history"][-1]["sigma"],
                             "switch_prob": got["history"][-1]["switch_prob"]}


@pytest.mark.parametrize("fit", [("amplitude", "sigma"), cfo.NAMES], ids=["default", "all_three"])
def test_loglikelihood_never_falls(fit):
    c, r = _planted_fit(2, fit)
    ll = [cfo.loglik(c["x"], c["chr_pos"], _levels(r, h), h["sigma"], h["switch_prob"]) for h in r["history"]]
    print(f"{r['n_iter']} iterations, converged {r['converged']}, log-likelihood {ll[0]:.6f} -> {ll[-1]:.6f}, "
          f"smallest step {np.diff(ll).min():.3g}")
    assert len(ll) == r["n_iter"] + 1 >= 3
    for before, after in zip(ll[:-1], ll[1:]):
        assert after - before >= -1e-9 * abs(before)  # (the slack of test_fit_oracle.py)
    assert ll[-1] > ll[0]


def test_loglik_is_the_log_of_the_sum_over_all_paths():
    import itertools

    x = np.array([[0.05, 0.31, 0.0, -0.2, 0.62]])
    mu, sigma, p = [-0.3, 0.0, 0.3, 0.6], 0.1, 0.05
    total = 0.0
    for path in itertools.product(range(4), repeat=x.shape[1]):
        wgt = 1.0 / 4.0
        for t, s in enumerate(path):
            wgt *= math.exp(-((x[0, t] - mu[s]) ** 2) / (2 * sigma * sigma)) / (sigma * math.sqrt(2 * math.pi))
            if t:
                wgt *= (1.0 - p) if path[t - 1] == s else p / 3.0
        total += wgt
    assert abs(cfo.loglik(sp.csr_matrix(x), {"c": 0}, mu, sigma, p) - math.log(total)) <= 1e-12 * abs(math.log(total)) + 1e-12


# ---- the planted case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_planted_levels_are_recovered_from_the_default_start(seed):
    c, r = _planted_fit(seed)
    calls = co.cnv_copy_states(c["x"], c["chr_pos"], **r["params"])[0]
    wrong = int((calls != c["truth"]).sum())
    print(f"seed {seed}: {wrong} wrong calls of {calls.size}, amplitude {r['amplitude']!r}, sigma "
          f"{r['params']['sigma']!r}, {r['n_iter']} iterations from {r['history'][0]}")
    assert wrong <= co.PLANTED_MOST_WRONG
    assert abs(r["amplitude"] - 0.3) <= 0.01 and abs(r["params"]["sigma"] - 0.1) <= 0.005 and r["converged"]
    assert wrong == cfo.PLANTED_WRONG[seed] and r["n_iter"] == cfo.PLANTED_N_ITER[seed]
    assert (r["amplitude"], r["params"]["sigma"]) == (cfo.PLANTED_AMPLITUDE[seed], cfo.PLANTED_SIGMA[seed])
    assert r["params"]["levels"] == [float(k) * r["amplitude"] for k in co.DEFAULT_STEPS] and r["params"]["switch_prob"] == 1e-3
    assert r["steps"] == list(co.DEFAULT_STEPS) and r["fit"] == ["amplitude", "sigma"]
    assert r["history"][-1] == {"amplitude": r["amplitude"], "sigma": r["params"]["sigma"], "switch_prob": 1e-3}
    # the start: the difference-based sigma (about 0.143; the root mean square is about 0.33) and twice that
    start = r["history"][0]
    assert 0.14 <= start["sigma"] <= 0.15 and start["amplitude"] == 2.0 * start["sigma"]
    # the true parameters do no better
    truth = co.cnv_copy_states(c["x"], c["chr_pos"], **c["kwargs"])[0]
    assert int((truth != c["truth"]).sum()) == wrong


@pytest.mark.parametrize("seed", range(5))
def test_the_rule_of_thumb_of_cnv_copy_states_misses_the_planted_levels(seed):
    """The documented reason for the fit: sigma = RMS and amplitude = 2 RMS leave at least 500 wrong calls."""
    c = co.planted_levels(seed)
    sigma = so.default_sigma(so.canonical(c["x"]))
    calls = co.cnv_copy_states(c["x"], c["chr_pos"], sigma=sigma, amplitude=2 * sigma)[0]
    wrong = int((calls != c["truth"]).sum())
    assert wrong >= 500 and wrong == cfo.PLANTED_RMS_START_WRONG[seed]
    assert np.array_equal(calls, co.cnv_copy_states(c["x"], c["chr_pos"])[0])  # (these are its defaults)


# ---- the M-step and the edge cases -------------------------------------------------------------------------------------------
def test_m_step_rules():
    steps, ks = (-1, 0, 2), [-1.0, 0.0, 2.0]
    Ns, Ms, Qs, N = [3.0, 10.0, 2.0], [-1.5, 0.25, 2.5], 9.0, 15.0
    num = math.fsum(k * m for k, m in zip(ks, Ms))
    den = math.fsum((k * k) * v for k, v in zip(ks, Ns))
    assert (num, den) == (6.5, 11.0)
    a, sigma, p = cfo.m_step(Ns, Ms, 9.0, Qs, N, 10, steps, 0.4, 0.2, 0.1, cfo.NAMES)
    assert a == 6.5 / 11.0
    mu = [k * a for k in ks]
    var = ((Qs - 2.0 * math.fsum(m * v for m, v in zip(mu, Ms))) + math.fsum((m * m) * v for m, v in zip(mu, Ns))) / N
    assert sigma == math.sqrt(var) and p == 1.0 - 9.0 / 10
    # the others keep their values; sigma then uses the amplitude it was given
    assert cfo.m_step(Ns, Ms, 9.0, Qs, N, 10, steps, 0.4, 0.2, 0.1, ["amplitude"]) == (a, 0.2, 0.1)
    kept = cfo.m_step(Ns, Ms, 9.0, Qs, N, 10, steps, 0.4, 0.2, 0.1, ["sigma"])
    mu = [k * 0.4 for k in ks]
    var = ((Qs - 2.0 * math.fsum(m * v for m, v in zip(mu, Ms))) + math.fsum((m * m) * v for m, v in zip(mu, Ns))) / N
    assert kept == (0.4, math.sqrt(var), 0.1)
    # amplitude stays when num or den is not positive; switch_prob is clamped and stays without a step
    assert cfo.m_step(Ns, [1.5, 0.0, 0.5], 9.0, Qs, N, 10, steps, 0.4, 0.2, 0.1, ["amplitude"])[0] == 0.4
    assert cfo.m_step([0.0, 15.0, 0.0], Ms, 9.0, Qs, N, 10, steps, 0.4, 0.2, 0.1, ["amplitude"])[0] == 0.4
    assert cfo.m_step(Ns, Ms, 10.0, Qs, N, 10, steps, 0.4, 0.2, 0.1, ["switch_prob"])[2] == cfo.P_MIN
    assert cfo.m_step(Ns, Ms, 2.0, Qs, N, 10, steps, 0.4, 0.2, 0.1, ["switch_prob"])[2] == cfo.P_MAX
    assert cfo.m_step(Ns, Ms, 2.0, Qs, N, 0, steps, 0.4, 0.2, 0.1, ["switch_prob"])[2] == 0.1
    # a variance that is not > 0 is a degenerate step
    assert cfo.m_step(Ns, Ms, 9.0, 0.0, N, 10, steps, 0.4, 0.2, 0.1, ["sigma"]) is None


def test_all_zero_matrix_returns_zero_levels_without_an_iteration():
    x, pos = sp.csr_matrix((4, 12)), {"c": 0, "d": 5}
    r = cfo.cnv_copy_states_fit(x, pos)
    stored = co.cnv_copy_states(x, pos)[3]
    assert r["params"] == {"levels": [0.0] * 6, "sigma": 0.0, "switch_prob": 1e-3}
    assert _bits(r["params"]["levels"]) == _bits(stored["levels"]) and r["params"]["sigma"] == stored["sigma"]
    assert r["n_iter"] == 0 and not r["converged"] and r["amplitude"] == 0.0
    assert r["history"] == [{"amplitude": 0.0, "sigma": 0.0, "switch_prob": 1e-3}]


@pytest.mark.parametrize("steps", [(-1, 0, 1), None], ids=["three_steps", "default_steps"])
def test_degenerate_step_stops_with_the_previous_parameters(steps):
    x, pos, kw = fo.degenerate_case()
    lattice = co.DEFAULT_STEPS if steps is None else steps
    s = cfo.stats(x, pos, cfo.levels_of(lattice, 0.5), 1e-3, 1e-3)
    k = len(lattice)
    assert np.isfinite(s).all() and s[:, :k].sum() == x.shape[0] * x.shape[1]
    r = cfo.cnv_copy_states_fit(x, pos, steps=steps, **kw)
    assert r["stopped"] == "degenerate" and not r["converged"] and r["n_iter"] == 1
    assert r["history"] == [{"amplitude": 0.5, "sigma": 1e-3, "switch_prob": 1e-3}]
    assert r["params"] == {"levels": cfo.levels_of(lattice, 0.5), "sigma": 1e-3, "switch_prob": 1e-3}
    # fitting the amplitude alone is not degenerate: nothing divides by the variance
    r = cfo.cnv_copy_states_fit(x, pos, steps=steps, fit=("amplitude",), **kw)
    assert "stopped" not in r and r["converged"] and r["amplitude"] == 0.5


def test_one_window_only_has_no_pair_and_no_step():
    """No chromosome has two windows: the start sigma falls back to the root mean square, S is 0 and switch_prob stays."""
    c = co.shapes()["one_window"]
    x = so.canonical(c["x"])
    assert x.shape[1] == 1 and cfo._n_steps(c["chr_pos"], *x.shape) == 0
    assert cfo.start_sigma(x, c["chr_pos"]) == so.default_sigma(x) > 0.0
    r = cfo.cnv_copy_states_fit(c["x"], c["chr_pos"], fit=cfo.NAMES, switch_prob=0.02)
    assert r["n_iter"] >= 1 and all(h["switch_prob"] == 0.02 for h in r["history"])
    assert r["history"][0]["sigma"] == so.default_sigma(x)
    s = cfo.stats(c["x"], c["chr_pos"], cfo.levels_of(co.DEFAULT_STEPS, 0.3), 0.1, 0.02)
    assert (s[:, 12] == 0.0).all()
    # a matrix whose adjacent windows are all equal has differences of 0: the root mean square as well
    flat = np.full((3, 7), 0.25)
    assert cfo.start_sigma(so.canonical(flat), {"a": 0}) == 0.25


def test_one_window_chromosome_between_long_adds_its_sums_in_chromosome_order():
    c = co.shapes()["one_window_chromosome_between_long"]
    x = so.canonical(c["x"])
    mu, sigma, p = cfo.levels_of(co.DEFAULT_STEPS, 0.3), 0.1, 1e-3
    whole = cfo.stats(x, c["chr_pos"], mu, sigma, p)
    parts = [cfo.stats(x[:, a:b], {"a": 0}, mu, sigma, p) for a, b in ((0, 30), (30, 31), (31, 61))]
    assert _bits(whole) == _bits((parts[0] + parts[1]) + parts[2])
    assert (parts[1][:, 12] == 0.0).all() and np.abs(parts[1][:, :6].sum(axis=1) - 1.0).max() <= STAT_REL


def test_start_values_whose_emission_overflows_raise():
    x, pos, kw = so.overflow_case()
    with pytest.raises(ValueError, match="overflow"):
        cfo.cnv_copy_states_fit(x, pos, **kw)
    mu = cfo.levels_of(co.DEFAULT_STEPS, kw["amplitude"])
    x.data[np.abs(x.data) > 1e100] = co.largest_value_that_does_not_overflow(mu, kw["sigma"])
    assert cfo.cnv_copy_states_fit(x, pos, max_iter=1, **kw)["n_iter"] == 1


# ---- the library and the package, as far as they go without a GPU -------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    name = "icv_copy_posterior_stats"
    assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
    assert f"lib.load().{name}" in open(os.path.join(ROOT, "infercnvpy_amd", "_engine.py")).read()
    assert callable(_engine.copy_posterior_stats)
    assert "cnv_copy_states_fit" in cnv.tl.__all__ and callable(cnv.tl.cnv_copy_states_fit)
    assert re.search(r"#define\s+ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS\(k, n_chr\)", header)
    assert re.search(r"#define\s+ICV_COPY_POSTERIOR_STATS_LDS\(n_cols, k, n_chr\)", header)
    for k in range(cpo.MIN_STATES, cpo.MAX_STATES + 1):
        for n_chr in (1, 23, 65, 130):
            cap = _lib.ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(k, n_chr)
            assert cap == cfo.max_windows(k, n_chr) <= _lib.ICV_COPY_POSTERIOR_MAX_WINDOWS(k)
            assert _lib.ICV_COPY_POSTERIOR_STATS_LDS(cap, k, n_chr) == cfo.lds_bytes(cap, k, n_chr) <= 163840
            assert _lib.ICV_COPY_POSTERIOR_STATS_LDS(cap + 1, k, n_chr) > _lib.ICV_COPY_POSTERIOR_LDS_BYTES == 163840
    assert _lib.ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(6, 1) == (163840 - 8 * 13) // 56 == 2923
    assert _lib.ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(8, 2000) == 0  # the sums of the chromosomes alone fill the LDS


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: every call below fails in the argument checks (or has no rows)
    six = [k * 0.3 for k in co.DEFAULT_STEPS]
    ok = dict(levels=six, neutral=2, h=50.0, ps=0.999, pw=0.0002)

    def matrix(n_cols):
        m = _lib.Matrix(format=_lib.ICV_CSR, dtype=_lib.ICV_F64, n_rows=0, n_cols=n_cols, ld=n_cols)
        m.indptr = 16
        return m

    def stats(mat, n_chr=1, chr_start=one, out=one, no_levels=False, **kw):
        a = dict(ok, **kw)
        mu = None if no_levels else (ctypes.c_double * len(a["levels"]))(*a["levels"])
        return lib.icv_copy_posterior_stats(ctypes.byref(mat) if mat is not None else None, chr_start, n_chr, mu,
                                            len(a["levels"]), a["neutral"], a["h"], a["ps"], a["pw"], out, None)

    def error():
        return lib.icv_last_error().decode()

    m = matrix(8)
    assert stats(m) == _lib.ICV_OK  # no rows: nothing is launched
    for bad in (dict(mat=None), dict(mat=m, chr_start=None), dict(mat=m, out=None), dict(mat=m, no_levels=True),
                dict(mat=m, n_chr=0)):
        assert stats(**bad) == _lib.ICV_ERR_INVALID, bad
        assert error() == "bad copy_posterior_stats arguments"
    assert stats(matrix(0)) == _lib.ICV_ERR_INVALID and "n_cols = 0 must lie in" in error()
    assert stats(m, n_chr=9) == _lib.ICV_ERR_INVALID and "more chromosomes than windows" in error()
    for kw, rule in (({"levels": [0.0]}, "n_levels"), ({"levels": [float(k) for k in range(9)], "neutral": 0}, "n_levels"),
                     ({"neutral": 6}, "neutral"), ({"neutral": -1}, "neutral"),
                     ({"levels": [-0.3, 0.0, math.inf], "neutral": 1}, "finite"),
                     ({"levels": [-0.3, 0.0, 0.0], "neutral": 1}, "ascend"), ({"neutral": 1}, "must be 0"),
                     ({"h": math.inf}, "h must be"), ({"h": 0.0}, "h must be"), ({"ps": 1.0}, "ps ="),
                     ({"ps": math.nan}, "ps ="), ({"pw": 0.0}, "ps ="), ({"pw": 1e-320}, "ps =")):
        assert stats(m, **kw) == _lib.ICV_ERR_INVALID, kw
        assert rule in error(), (kw, error())
    # the order: the pointers, the window range, the chromosomes, the model, the matrix
    assert stats(matrix(0), n_chr=0, neutral=9) == _lib.ICV_ERR_INVALID and error() == "bad copy_posterior_stats arguments"
    assert stats(matrix(0), neutral=9) == _lib.ICV_ERR_INVALID and "n_cols" in error()
    assert stats(m, n_chr=9, neutral=9) == _lib.ICV_ERR_INVALID and "more chromosomes" in error()
    broken = matrix(8)
    broken.indptr = None
    assert stats(broken, neutral=9) == _lib.ICV_ERR_INVALID and "neutral" in error()
    assert stats(broken) == _lib.ICV_ERR_INVALID and "incomplete matrix" in error()
    # the same calls get the same verdicts from icv_copy_posterior_chains, whose checks these are

    def chains(mat, n_chr=1, **kw):
        a = dict(ok, **kw)
        mu = (ctypes.c_double * len(a["levels"]))(*a["levels"])
        return lib.icv_copy_posterior_chains(ctypes.byref(mat), one, n_chr, mu, len(a["levels"]), a["neutral"], a["h"],
                                             a["ps"], a["pw"], one, None, None)

    for args, kw, rule in (((matrix(0),), {"neutral": 9}, "n_cols = 0 must lie in"), ((m, 9), {"neutral": 9}, "more chromosomes"),
                           ((broken,), {"neutral": 9}, "neutral must be"), ((broken,), {"pw": 0.0}, "ps = 1 - p"),
                           ((broken,), {}, "incomplete matrix")):
        for entry in (chains, stats):
            assert entry(*args, **kw) == _lib.ICV_ERR_INVALID and rule in error(), (entry.__name__, kw, error())


def test_c_abi_refuses_a_shape_over_the_lds_bound():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(16)
    six = (ctypes.c_double * 6)(*[k * 0.3 for k in co.DEFAULT_STEPS])

    def stats(n_cols, n_chr, mu=six, k=6, neutral=2):
        m = _lib.Matrix(format=_lib.ICV_CSR, dtype=_lib.ICV_F64, n_rows=0, n_cols=n_cols, ld=n_cols)
        m.indptr = 16
        return lib.icv_copy_posterior_stats(ctypes.byref(m), one, n_chr, mu, k, neutral, 50.0, 0.999, 0.0002, one, None)

    assert stats(2923, 1) == _lib.ICV_OK
    assert stats(2924, 1) == _lib.ICV_ERR_INVALID
    msg = lib.icv_last_error().decode()
    assert "2923" in msg and "163840" in msg and "K = 6" in msg
    # icv_copy_posterior_chains takes 3 413 windows with K = 6; here the chromosomes' sums take their share
    assert stats(2883, 23) == _lib.ICV_OK and stats(2884, 23) == _lib.ICV_ERR_INVALID
    assert stats(cfo.max_windows(6, 130), 130) == _lib.ICV_OK
    assert stats(cfo.max_windows(6, 130) + 1, 130) == _lib.ICV_ERR_INVALID
    two = (ctypes.c_double * 2)(0.0, 0.3)
    assert stats(cfo.max_windows(2, 1), 1, two, 2, 0) == _lib.ICV_OK
    assert stats(cfo.max_windows(2, 1) + 1, 1, two, 2, 0) == _lib.ICV_ERR_INVALID
    eight = (ctypes.c_double * 8)(*[(s - 3) * 0.3 for s in range(8)])
    assert stats(cfo.max_windows(8, 1), 1, eight, 8, 3) == _lib.ICV_OK
    assert stats(cfo.max_windows(8, 1) + 1, 1, eight, 8, 3) == _lib.ICV_ERR_INVALID


def _adata(n=4, w=10, chr_pos=None, x=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def test_missing_keys_and_bad_arguments_raise_before_anything_touches_a_device():
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(KeyError, match="X_other not found in adata.obsm. Did you run `tl.infercnv`"):
        cnv.tl.cnv_copy_states_fit(ad, use_rep="other")
    for kw, match in (({"steps": (-1, 1, 2)}, "must hold 0"), ({"steps": (1, 0, -1)}, "ascend"),
                      ({"steps": (0, 1, 1)}, "ascend"), ({"steps": (-1, 0, 1.5)}, "integers"),
                      ({"steps": (0, "x")}, "integers"), ({"steps": (0, True)}, "integers"), ({"steps": 3}, "sequence"),
                      ({"steps": (0,)}, "1 states"), ({"steps": tuple(range(-4, 5))}, "9 states"),
                      ({"fit": ("amplitude", "levels")}, "fit"), ({"fit": ()}, "fit"), ({"fit": 3}, "fit"),
                      ({"max_iter": 0}, "max_iter"), ({"max_iter": 2.0}, "max_iter"), ({"max_iter": True}, "max_iter"),
                      ({"tol": np.nan}, "tol"), ({"tol": -1e-3}, "tol"), ({"tol": np.inf}, "tol"), ({"tol": "x"}, "tol"),
                      ({"amplitude": 0.0}, "amplitude"), ({"sigma": -1.0}, "sigma"), ({"sigma": np.nan}, "sigma"),
                      ({"switch_prob": 0.0}, "switch_prob"), ({"switch_prob": 1.0}, "switch_prob"),
                      ({"switch_prob": True}, "switch_prob"), ({"switch_prob": 1e-320}, "too close"),
                      ({"switch_prob": 5e-308}, "too close")):
        with pytest.raises(ValueError, match="tl.cnv_copy_states_fit: .*" + match):
            cnv.tl.cnv_copy_states_fit(ad, **kw)
    with pytest.raises(ValueError, match="outside"):
        cnv.tl.cnv_copy_states_fit(_adata(chr_pos={"chr1": 0, "chr2": 10}))
    # the LDS bound: 2 923 windows for K = 6 in one chromosome, fewer in two
    with pytest.raises(ValueError, match="163840.*at most 2923"):
        cnv.tl.cnv_copy_states_fit(_adata(n=1, x=sp.csr_matrix((1, 2924)), chr_pos={"chr1": 0}))
    with pytest.raises(ValueError, match="2923 windows in 2 chromosomes.*163840.*at most 2922 windows"):
        cnv.tl.cnv_copy_states_fit(_adata(n=1, x=sp.csr_matrix((1, 2923)), chr_pos={"chr1": 0, "chr2": 5}))
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match="chr_pos not found"):
        cnv.tl.cnv_copy_states_fit(ad)
    assert "cnv_copy_states_fit" not in ad.uns

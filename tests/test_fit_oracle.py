"""The oracle of tl.cnv_states_fit (tests/_fit_oracle.py) against a hand computation and the properties
of expectation-maximisation, and everything of the function that needs no GPU: the C ABI and the export."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _fit_oracle as fo
import _posterior_oracle as po
import _states_oracle as so
from _tsne_oracle import exp_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (60, [30, 7, 41, 1, 22], 5)  # the planted matrix of the trajectory tests


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


def _exp(v):
    return float(exp_(np.float64(v)))


def test_two_window_chain_by_hand():
    """G, D and K of one chain of two windows from the rules, one Python-float operation per written operation."""
    a, sigma, p = 0.5, 0.25, 0.25
    h, ps, pw = 1.0 / (2.0 * sigma * sigma), 1.0 - p, p / 2.0
    assert (h, ps, pw) == (8.0, 0.75, 0.125)
    x0, x1 = 0.375, -0.125

    def emit(x):
        e = []
        for mu in (-a, 0.0, a):
            t = x - mu
            e.append(-(t * t) * h)
        m = max(e)
        return [_exp(v - m) for v in e]

    b0, b1 = emit(x0), emit(x1)
    # forward
    c0 = (b0[0] + b0[1]) + b0[2]
    al0 = [b0[s] / c0 for s in range(3)]
    pred = [((al0[0] * ps) + (al0[1] * pw)) + (al0[2] * pw), ((al0[0] * pw) + (al0[1] * ps)) + (al0[2] * pw),
            ((al0[0] * pw) + (al0[1] * pw)) + (al0[2] * ps)]
    u = [pred[s] * b1[s] for s in range(3)]
    c1 = (u[0] + u[1]) + u[2]
    al1 = [u[s] / c1 for s in range(3)]
    # t = 1: be = 1
    w = [al1[s] * 1.0 for s in range(3)]
    z1 = (w[0] + w[1]) + w[2]
    gam = [w[s] / z1 for s in range(3)]
    G = 0.0 + (gam[0] + gam[2])
    D = 0.0 + (gam[2] - gam[0]) * x1
    # t = 0
    g = [b1[s] * 1.0 for s in range(3)]
    v = [((ps * g[0]) + (pw * g[1])) + (pw * g[2]), ((pw * g[0]) + (ps * g[1])) + (pw * g[2]),
         ((pw * g[0]) + (pw * g[1])) + (ps * g[2])]
    be0 = [v[r] / c1 for r in range(3)]
    w = [al0[s] * be0[s] for s in range(3)]
    z0 = (w[0] + w[1]) + w[2]
    gam = [w[s] / z0 for s in range(3)]
    G = G + (gam[0] + gam[2])
    D = D + (gam[2] - gam[0]) * x0
    m = [(al0[s] * ps) * g[s] for s in range(3)]
    st = (m[0] + m[1]) + m[2]
    K = 0.0 + (st / c1) / z0

    got = fo.chain_stats(np.array([[x0, x1]]), a, h, ps, pw)
    assert [_bits(t)[0] for t in got] == _bits([G, D, K])
    assert 0.0 < G < 2.0 and 0.0 < K < 1.0 and D != 0.0
    whole = fo.stats(sp.csr_matrix(np.array([[x0, x1]])), {"c": 0}, a, sigma, p)
    assert _bits(whole[0]) == _bits([G, D, K])
    # two chromosomes of one window: no step, and the cell's sums add the chromosomes in ascending order
    split = fo.stats(sp.csr_matrix(np.array([[x0, x1]])), {"c": 0, "d": 1}, a, sigma, p)
    one = [fo.chain_stats(np.array([[v]]), a, h, ps, pw) for v in (x0, x1)]
    assert split[0, 2] == 0.0
    assert _bits(split[0, :2]) == _bits([(0.0 + one[0][k][0]) + one[1][k][0] for k in range(2)])


def test_stay_mass_and_altered_mass_are_what_the_posteriors_say():
    """G and D against the gamma planes of the posterior oracle, K against the pairwise posteriors summed over the
    diagonal, computed independently from al, be, b and c in float64 (bound 1e-12 per cell: a wrong formula is off by
    far more, rounding by far less)."""
    c = so.planted(5, [9, 1, 14], 2)
    a, sigma, p = 0.2, 0.1, 0.01
    got = fo.stats(c["x"], c["chr_pos"], a, sigma, p)
    loss, neutral, gain, _ = po.cnv_posteriors(c["x"], c["chr_pos"], amplitude=a, sigma=sigma, switch_prob=p)
    dense = c["x"].toarray()
    assert np.abs(got[:, 0] - (loss + gain).sum(axis=1)).max() <= 1e-12
    assert np.abs(got[:, 1] - ((gain - loss) * dense).sum(axis=1)).max() <= 1e-12
    # K <= the number of steps, and K + expected switches = steps: with p -> 0 nearly every step stays
    n_steps = fo.steps(c["chr_pos"], 1, dense.shape[1])
    assert n_steps == 8 + 0 + 13
    assert (got[:, 2] > 0.0).all() and (got[:, 2] <= n_steps * (1 + 1e-12)).all()
    sticky = fo.stats(c["x"], c["chr_pos"], a, sigma, 1e-12)
    assert np.abs(sticky[:, 2] - n_steps).max() <= 1e-6
    # the pairwise posterior by brute force over all 3^T paths of a short chain
    x = [0.05, 0.31, 0.0, -0.2]
    h, ps, pw = po.scalars(sigma, p)
    mus = (-a, 0.0, a)
    stay = total = 0.0
    import itertools
    for path in itertools.product(range(3), repeat=len(x)):
        wgt = 1.0
        for t, s in enumerate(path):
            wgt *= math.exp(-((x[t] - mus[s]) ** 2) * h)
            if t:
                wgt *= ps if path[t - 1] == s else pw
        total += wgt
        stay += wgt * sum(path[t - 1] == path[t] for t in range(1, len(x)))
    K = fo.chain_stats(np.array([x]), a, h, ps, pw)[2][0]
    assert abs(K - stay / total) <= 1e-12


@functools.lru_cache(maxsize=None)
def _fit_small(fit):
    c = so.planted(*SMALL)
    return c, fo.cnv_states_fit(c["x"], c["chr_pos"], fit=fit)


def test_loglikelihood_never_falls():
    c, r = _fit_small(fo.NAMES)
    ll = [fo.loglik(c["x"], c["chr_pos"], **h) for h in r["history"]]
    steps = np.diff(ll)
    print(f"{r['n_iter']} iterations, converged {r['converged']}, log-likelihood {ll[0]:.6f} -> {ll[-1]:.6f}, "
          f"smallest step {steps.min():.3g}")
    assert len(ll) == r["n_iter"] + 1 >= 3
    for before, after in zip(ll[:-1], ll[1:]):
        assert after - before >= -1e-9 * abs(before)
    assert ll[-1] > ll[0]


def test_loglik_is_the_log_of_the_sum_over_all_paths():
    x = np.array([[0.05, 0.31, 0.0, -0.2, 0.22]])
    a, sigma, p = 0.2, 0.1, 0.05
    import itertools
    total = 0.0
    for path in itertools.product(range(3), repeat=x.shape[1]):
        wgt = 1.0 / 3.0
        for t, s in enumerate(path):
            wgt *= math.exp(-((x[0, t] - (-a, 0.0, a)[s]) ** 2) / (2 * sigma * sigma)) / (sigma * math.sqrt(2 * math.pi))
            if t:
                wgt *= (1.0 - p) if path[t - 1] == s else p / 2.0
        total += wgt
    assert abs(fo.loglik(sp.csr_matrix(x), {"c": 0}, a, sigma, p) - math.log(total)) <= 1e-12 * abs(math.log(total)) + 1e-12


def test_recovery_of_the_planted_parameters():
    c = so.planted(*SMALL, keep=0.0)  # unthresholded Gaussian noise of 0.1, segments shifted by 0.6
    r = fo.cnv_states_fit(c["x"], c["chr_pos"])
    print(f"fitted {r['params']} in {r['n_iter']} iterations")
    assert r["converged"] and r["n_iter"] <= 10 and r["fit"] == ["amplitude", "sigma"]
    assert abs(r["params"]["amplitude"] - 0.6) <= 0.03 * 0.6
    assert abs(r["params"]["sigma"] - 0.1) <= 0.03 * 0.1
    assert r["params"]["switch_prob"] == 1e-3
    assert len(r["history"]) == r["n_iter"] + 1 and r["history"][-1] == r["params"]
    assert r["history"][0] == so.cnv_states(c["x"], c["chr_pos"])[2]


def test_calls_with_the_fitted_parameters_are_closer_to_the_truth():
    c = so.planted(100, po.LENGTHS_1802, 3)
    r = fo.cnv_states_fit(c["x"], c["chr_pos"])
    default = so.cnv_states(c["x"], c["chr_pos"])[0]
    fitted = so.cnv_states(c["x"], c["chr_pos"], **r["params"])[0]
    wrong_default, wrong_fitted = int((default != c["truth"]).sum()), int((fitted != c["truth"]).sum())
    print(f"fitted {r['params']} in {r['n_iter']} iterations: {wrong_fitted} wrong calls against {wrong_default} of "
          f"{int((c['truth'] != 0).sum())} altered windows")
    assert r["converged"] and wrong_fitted < wrong_default


def test_fit_sigma_alone_keeps_the_other_two():
    c = so.planted(*SMALL)
    r = fo.cnv_states_fit(c["x"], c["chr_pos"], amplitude=0.55, switch_prob=0.01, fit=("sigma",))
    assert r["fit"] == ["sigma"] and r["n_iter"] >= 2
    for h in r["history"]:
        assert _bits([h["amplitude"], h["switch_prob"]]) == _bits([0.55, 0.01])
    assert r["params"]["sigma"] != r["history"][0]["sigma"]


def test_one_window_has_no_step_and_keeps_switch_prob():
    c = po._cases()["one_window"]()
    assert fo.steps(c["chr_pos"], *c["x"].shape) == 0
    r = fo.cnv_states_fit(c["x"], c["chr_pos"], fit=fo.NAMES, switch_prob=0.02)
    assert r["n_iter"] >= 1 and all(h["switch_prob"] == 0.02 for h in r["history"])
    assert (fo.stats(c["x"], c["chr_pos"], 0.2, 0.1, 0.02)[:, 2] == 0.0).all()


def test_switch_prob_is_clamped():
    assert fo.m_step(1.0, 1.0, 10.0, 5.0, 20.0, 10, 0.5, 0.2, 0.1, ["switch_prob"])[2] == fo.P_MIN  # every step stays
    assert fo.m_step(1.0, 1.0, 2.0, 5.0, 20.0, 10, 0.5, 0.2, 0.1, ["switch_prob"])[2] == fo.P_MAX
    assert fo.m_step(1.0, 1.0, 9.0, 5.0, 20.0, 10, 0.5, 0.2, 0.1, ["switch_prob"])[2] == 1.0 - 9.0 / 10
    # amplitude stays when the altered mass or the first moment is not positive
    assert fo.m_step(0.0, 0.0, 9.0, 5.0, 20.0, 10, 0.5, 0.2, 0.1, ["amplitude"])[0] == 0.5
    assert fo.m_step(2.0, -1.0, 9.0, 5.0, 20.0, 10, 0.5, 0.2, 0.1, ["amplitude"])[0] == 0.5
    assert fo.m_step(2.0, 1.0, 9.0, 5.0, 20.0, 10, 0.25, 0.2, 0.1, ["amplitude"])[0] == 0.5


def test_all_zero_matrix_returns_zeros_without_an_iteration():
    r = fo.cnv_states_fit(sp.csr_matrix((4, 12)), {"c": 0, "d": 5})
    assert r["params"] == {"amplitude": 0.0, "sigma": 0.0, "switch_prob": 1e-3} == r["history"][0]
    assert r["n_iter"] == 0 and len(r["history"]) == 1 and not r["converged"]
    assert r["params"] == so.cnv_states(sp.csr_matrix((4, 12)), {"c": 0, "d": 5})[2]


def test_degenerate_step_stops_with_the_previous_parameters():
    x, pos, kw = fo.degenerate_case()
    s = fo.stats(x, pos, 0.5, 1e-3, 1e-3)
    assert s[:, 0].sum() == x.nnz and s[:, 1].sum() == 0.5 * x.nnz and np.isfinite(s).all()
    r = fo.cnv_states_fit(x, pos, **kw)
    assert r["stopped"] == "degenerate" and not r["converged"] and r["n_iter"] == 1
    assert r["params"] == {"amplitude": 0.5, "sigma": 1e-3, "switch_prob": 1e-3} and r["history"] == [r["params"]]
    # fitting the amplitude alone is not degenerate: nothing divides by the variance
    r = fo.cnv_states_fit(x, pos, fit=("amplitude",), **kw)
    assert "stopped" not in r and r["converged"] and r["params"]["amplitude"] == 0.5


@pytest.mark.parametrize("name", po.CASE_NAMES)
def test_statistics_of_every_case_are_finite(name):
    c = po._cases()[name]()  # (the case without its expected posteriors, which are not needed here)
    kw = c["kwargs"]
    sigma = kw.get("sigma", so.default_sigma(c["x"]))
    x = c["x"][:8]
    s = fo.stats(x, c["chr_pos"], kw.get("amplitude", 2.0 * sigma), sigma, kw.get("switch_prob", 1e-3))
    assert s.shape == (x.shape[0], 3) and np.isfinite(s).all() and (s[:, 0] >= 0.0).all() and (s[:, 2] >= 0.0).all()


# ---- the library and the package, as far as they go without a GPU -------------------------------------------------------------
def test_symbol_is_exported_and_declared():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    assert "icv_posterior_stats" in declared and "icv_posterior_stats" in _lib.EXPORTS
    assert hasattr(lib, "icv_posterior_stats")
    assert "cnv_states_fit" in cnv.tl.__all__ and callable(cnv.tl.cnv_states_fit)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    m = _lib.Matrix(format=_lib.ICV_CSR, dtype=_lib.ICV_F64, n_rows=0, n_cols=8, ld=8)
    one = ctypes.c_void_p(16)  # never dereferenced: every call below fails in the argument checks (or has no rows)
    ok = dict(amplitude=1.0, h=2.0, ps=0.999, pw=0.0005)

    def stats(mat, n_chr=1, chr_start=one, out=one, **kw):
        a = dict(ok, **kw)
        return lib.icv_posterior_stats(ctypes.byref(mat) if mat is not None else None, chr_start, n_chr, a["amplitude"],
                                       a["h"], a["ps"], a["pw"], out, None)

    m.indptr = 16
    assert stats(m) == _lib.ICV_OK  # no rows: nothing is launched
    assert stats(None) == _lib.ICV_ERR_INVALID
    assert stats(m, chr_start=None) == _lib.ICV_ERR_INVALID
    assert stats(m, out=None) == _lib.ICV_ERR_INVALID
    assert stats(m, n_chr=0) == _lib.ICV_ERR_INVALID
    assert stats(m, n_chr=9) == _lib.ICV_ERR_INVALID
    for kw in ({"amplitude": 0.0}, {"h": math.inf}, {"pw": 1e-320}, {"pw": 0.0}, {"ps": 1.0}, {"ps": math.nan}):
        assert stats(m, **kw) == _lib.ICV_ERR_INVALID, kw
    none = _lib.Matrix(format=_lib.ICV_CSR, dtype=_lib.ICV_F64, n_rows=0, n_cols=0, ld=0)
    none.indptr = 16
    assert stats(none) == _lib.ICV_ERR_INVALID
    wide = _lib.Matrix(format=_lib.ICV_CSR, dtype=_lib.ICV_F64, n_rows=0, n_cols=_lib.ICV_POSTERIOR_MAX_WINDOWS + 1, ld=0)
    wide.indptr = 16
    assert stats(wide) == _lib.ICV_ERR_INVALID
    assert str(_lib.ICV_POSTERIOR_MAX_WINDOWS) in lib.icv_last_error().decode()


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
        cnv.tl.cnv_states_fit(ad, use_rep="other")
    for kw, match in (({"amplitude": 0.0}, "amplitude"), ({"sigma": -1.0}, "sigma"), ({"sigma": np.nan}, "sigma"),
                      ({"switch_prob": 0.0}, "switch_prob"), ({"switch_prob": 1.0}, "switch_prob"),
                      ({"switch_prob": True}, "switch_prob"), ({"switch_prob": 1e-320}, "too close"),
                      ({"fit": ("amplitude", "mean")}, "fit"), ({"fit": ()}, "fit"), ({"fit": 3}, "fit"),
                      ({"max_iter": 0}, "max_iter"), ({"max_iter": 2.0}, "max_iter"), ({"max_iter": True}, "max_iter"),
                      ({"tol": np.nan}, "tol"), ({"tol": -1e-3}, "tol"), ({"tol": np.inf}, "tol"), ({"tol": "x"}, "tol")):
        with pytest.raises(ValueError, match=match):
            cnv.tl.cnv_states_fit(ad, **kw)
    with pytest.raises(ValueError, match="outside"):
        cnv.tl.cnv_states_fit(_adata(chr_pos={"chr1": 0, "chr2": 10}))
    cap = po.MAX_WINDOWS
    with pytest.raises(ValueError, match=str(cap)):
        cnv.tl.cnv_states_fit(_adata(n=1, x=sp.csr_matrix((1, cap + 1)), chr_pos={"chr1": 0}))
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match="chr_pos not found"):
        cnv.tl.cnv_states_fit(ad)
    assert "cnv_states_fit" not in ad.uns


def test_start_values_whose_emission_overflows_raise():
    x, pos, kw = so.overflow_case()
    with pytest.raises(ValueError, match="overflow"):
        fo.cnv_states_fit(x, pos, **kw)
    x.data[x.data == 1e160] = 1e154  # the sum of squares is finite, the emission is not
    assert math.isfinite(math.fsum(so.rowsq(x)))
    with pytest.raises(ValueError, match="overflow"):
        fo.cnv_states_fit(x, pos, **kw)
    x.data[x.data == 1e154] = so.largest_value_that_does_not_overflow(kw["amplitude"], kw["sigma"])
    assert fo.cnv_states_fit(x, pos, max_iter=1, **kw)["n_iter"] == 1


def test_stats_bounds_entry_point_adds_nothing_for_an_empty_chromosome():
    c = so.planted(6, [10, 7, 13], 19)
    want = fo.stats(c["x"], c["chr_pos"], 0.2, 0.1, 1e-3)
    assert _bits(fo.stats(c["x"], None, 0.2, 0.1, 1e-3, bounds=[0, 10, 10, 17, 30])) == _bits(want)
    part = fo.stats(c["x"], None, 0.2, 0.1, 1e-3, bounds=[3, 9, 28])
    alone = fo.stats(c["x"][:, 3:28], {"a": 0, "b": 6}, 0.2, 0.1, 1e-3)
    assert _bits(part) == _bits(alone)

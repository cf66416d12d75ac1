"""The oracle of tl.cnv_posteriors / tl.cnv_states_filter (tests/_posterior_oracle.py) against
independent computations, and everything of the two functions that needs no GPU: arguments, caps, the C ABI."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _posterior_oracle as po
import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = (1e-3, 1e-6, 0.3, 1e-12)


def _chain_inputs(rng, T, outliers=True):
    """One chain in the style of X_cnv: 60 % zeros, noise of 0.1, now and then a value 50 times as large."""
    x = rng.normal(0.0, 0.1, size=T)
    x[rng.random(T) < 0.6] = 0.0
    if outliers:
        far = rng.random(T) < 0.05
        x[far] *= 50.0
    return x


def _brute_force(x, a, sigma, p):
    """Posteriors of one chain from all 3^T paths: exact Gaussian emission densities (up to a common factor), path
    weights summed by math.fsum."""
    T = len(x)
    mus = (-a, 0.0, a)
    # scaled per window by the largest emission, which cancels in the posterior
    logs = [[-((v - mu) ** 2) / (2.0 * sigma * sigma) for mu in mus] for v in x]
    em = [[math.exp(l - max(row)) for l in row] for row in logs]
    ps, pw = 1.0 - p, p / 2.0
    weights = {(t, s): [] for t in range(T) for s in range(3)}
    total = []
    for path in itertools.product(range(3), repeat=T):
        wgt = em[0][path[0]]
        for t in range(1, T):
            wgt *= (ps if path[t - 1] == path[t] else pw) * em[t][path[t]]
        total.append(wgt)
        for t in range(T):
            weights[(t, path[t])].append(wgt)
    z = math.fsum(total)
    return np.array([[math.fsum(weights[(t, s)]) / z for t in range(T)] for s in range(3)])


def _oracle_chain(x, a, sigma, p):
    h, ps, pw = po.scalars(sigma, p)
    with np.errstate(all="ignore"):
        return po.chain(np.asarray(x, dtype=np.float64)[None, :], a, h, ps, pw)[:, 0, :]


def test_brute_force_over_all_paths():
    rng = np.random.default_rng(2024)
    worst = 0.0
    for k in range(200):
        T = int(rng.integers(1, 8))
        p = SWITCH[k % 4]
        x = _chain_inputs(rng, T)
        got = _oracle_chain(x, 0.2, 0.1, p)
        worst = max(worst, float(np.abs(got - _brute_force(x.tolist(), 0.2, 0.1, p)).max()))
    far = [0.0, 5.0, 0.0, -5.0, -5.0, 0.05, 5.0]  # 50 sigma: the other two emissions vanish
    for p in SWITCH:
        worst = max(worst, float(np.abs(_oracle_chain(far, 0.2, 0.1, p) - _brute_force(far, 0.2, 0.1, p)).max()))
    print(f"largest |oracle - brute force| = {worst:.3g}")
    assert worst <= 1e-12


def _logsumexp(v):
    m = max(v)
    if m == -np.inf:
        return m
    return m + np.log(sum(np.exp(u - m) for u in v))


def _log_space(x, a, sigma, p):
    """Forward-backward in log space with np.longdouble."""
    L = np.longdouble
    T = len(x)
    mus = (L(-a), L(0.0), L(a))
    h = L(1.0) / (L(2.0) * L(sigma) * L(sigma))
    le = [[-((L(v) - mu) ** 2) * h for mu in mus] for v in x]
    lps, lpw = np.log(L(1.0) - L(p)), np.log(L(p) / L(2.0))
    lt = [[lps if r == s else lpw for s in range(3)] for r in range(3)]
    fw = [le[0]]
    for t in range(1, T):
        fw.append([_logsumexp([fw[-1][r] + lt[r][s] for r in range(3)]) + le[t][s] for s in range(3)])
    bw = [[L(0.0)] * 3]
    for t in range(T - 2, -1, -1):
        bw.insert(0, [_logsumexp([lt[r][s] + le[t + 1][s] + bw[0][s] for s in range(3)]) for r in range(3)])
    out = np.empty((3, T))
    for t in range(T):
        lw = [fw[t][s] + bw[t][s] for s in range(3)]
        z = _logsumexp(lw)
        for s in range(3):
            out[s, t] = float(np.exp(lw[s] - z))
    return out


def test_long_chains_against_extended_precision_log_space():
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in range(24):
        T = int(rng.integers(8, 201)) if k else 200
        p = SWITCH[k % 4]
        x = _chain_inputs(rng, T)
        got = _oracle_chain(x, 0.2, 0.1, p)
        worst = max(worst, float(np.abs(got - _log_space(x.tolist(), 0.2, 0.1, p)).max()))
    print(f"largest |oracle - log-space longdouble| = {worst:.3g}")
    assert worst <= 1e-12


def test_posteriors_lie_in_0_1_and_sum_to_one():
    rng = np.random.default_rng(3)
    for k in range(40):
        x = _chain_inputs(rng, int(rng.integers(1, 201)))
        g = _oracle_chain(x, 0.2, 0.1, SWITCH[k % 4])
        assert np.isfinite(g).all() and (g >= 0.0).all() and (g <= 1.0).all()
        total = (g[0] + g[1]) + g[2]
        assert (np.abs(total - 1.0) <= 4 * np.finfo(np.float64).eps).all()
    c = po.case("outliers")
    for k in ("loss", "neutral", "gain"):
        assert (c[k] >= 0.0).all() and (c[k] <= 1.0).all()
    assert (c["gain"] == 1.0).any() and (c["neutral"] == 0.0).any() and (c["loss"] == 1.0).any()


def test_chains_do_not_cross_chromosomes_and_all_zero_is_neutral():
    c = so.planted(4, [9, 5], 1)
    loss, neutral, gain, params = po.cnv_posteriors(c["x"], c["chr_pos"])
    dense = c["x"].toarray()
    for lo, hi in ((0, 9), (9, 14)):
        alone = po.cnv_posteriors(sp.csr_matrix(dense[:, lo:hi]), {"c": 0}, **params)
        assert np.array_equal(alone[1], neutral[:, lo:hi]) and np.array_equal(alone[0], loss[:, lo:hi])
    zl, zn, zg, zp = po.cnv_posteriors(sp.csr_matrix((3, 7)), {"c": 0})
    assert (zn == 1.0).all() and not zl.any() and not zg.any() and zp["sigma"] == 0.0


def test_exp_cutoff_case_sits_on_the_cutoff_of_the_written_exponential():
    from _tsne_oracle import exp_

    assert float(exp_(np.float64(-708.0))) > 0.0 and float(exp_(np.nextafter(np.float64(-708.0), -np.inf))) == 0.0
    c = po.case("exp_cutoff")
    kw = c["kwargs"]
    h = po.scalars(kw["sigma"], kw["switch_prob"])[0]
    assert h == 8.0
    for v, want in zip(po.CUTOFF_VALUES, (-707.0, -708.0, -709.0)):
        e = [-((v - mu) * (v - mu)) * h for mu in (-kw["amplitude"], 0.0, kw["amplitude"])]
        assert e[1] - e[2] == want and np.float32(v) == v
    for k in ("loss", "neutral", "gain"):
        assert np.isfinite(c[k]).all() and (c[k] >= 0.0).all() and (c[k] <= 1.0).all()
    seen = {v: [] for v in po.CUTOFF_VALUES}
    for row, t, v in c["probes"]:
        seen[v].append(float(c["neutral"][row, t]))
    print({v: (min(p), max(p)) for v, p in seen.items()})
    assert all(len(p) == 2 * len(po.CUTOFF_PROBES) for p in seen.values())
    assert all(0.0 < p < 1e-300 for p in seen[88.625]) and all(0.0 < p < 1e-300 for p in seen[88.75])
    assert all(p == 0.0 for p in seen[88.875])
    assert any(p < 2.2250738585072014e-308 for p in seen[88.75])  # pred b went subnormal on the way
    starts = sorted(c["chr_pos"].values())
    assert [po.CUTOFF_PROBES[i] in starts for i in range(4)] == [True, False, False, True]
    assert po.CUTOFF_PROBES[2] + 1 == c["x"].shape[1] and starts[1] == 9 and starts[2] == 10  # window 9 is alone


def test_posterior_bounds_entry_point_and_overflow():
    c = so.planted(6, [10, 7, 13], 19)
    x = c["x"]
    kw = {"amplitude": 0.2, "sigma": 0.1, "switch_prob": 1e-3}
    want = po.cnv_posteriors(x, c["chr_pos"], **kw)
    for b in ([0, 10, 17, 30], [0, 10, 10, 17, 30]):
        got = po.cnv_posteriors(x, None, bounds=b, **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
    loss, neutral, gain, _ = po.cnv_posteriors(x, None, bounds=[3, 9, 28], **kw)
    for lo, hi in ((0, 3), (28, 30)):
        assert (neutral[:, lo:hi] == 1.0).all() and not loss[:, lo:hi].any() and not gain[:, lo:hi].any()
    assert np.array_equal(neutral[:, 9:28], po.cnv_posteriors(x[:, 9:28], {"c": 0}, **kw)[1])
    # the defect the overflow rule closes: rules 1-6 alone give 0 / 0 on the whole chromosome
    x, pos, kw = so.overflow_case()
    h, ps, pw = po.scalars(kw["sigma"], 1e-3)
    with np.errstate(all="ignore"):
        assert np.isnan(po.chain(x.toarray(), kw["amplitude"], h, ps, pw)).all()
    with pytest.raises(ValueError, match="overflow"):
        po.cnv_posteriors(x, pos, **kw)
    m = so.largest_value_that_does_not_overflow(kw["amplitude"], kw["sigma"])
    x.data[x.data == 1e160] = m
    assert all(np.isfinite(v).all() for v in po.cnv_posteriors(x, pos, **kw)[:3])


# ---- the filter's crafted cases have the power they are meant to have --------------------------------------------------------
def _rows_changed(c, variant, thr=None):
    thr = c["max_p_normal"] if thr is None else thr
    want = po.states_filter(c["states"], c["p"], c["chr_pos"], thr)[0]
    got = po.states_filter(c["states"], c["p"], c["chr_pos"], thr, variant)[0]
    return int((got != want).any(axis=1).sum())


@pytest.mark.parametrize("neighbourhood", po.SWEEP_NEIGHBOURHOODS)
def test_step_boundary_sweep_has_both_verdicts_and_sees_a_lost_window(neighbourhood):
    """Rows whose filtered calls change when a window is lost, measured on the CPU for drop_first / drop_first_sum /
    drop_64 / drop_64_sum: alone 85 / 85 / 51 / 70 of 171, behind_other_sign 79 / 109 / 67 / 81 of 153,
    before_same_sign_chromosome 112 / 153 / 80 / 75 of 153."""
    cases = po.sweep_cases(neighbourhood)
    rows = sum(len(c["main"]) for c in cases)
    goes = stays = 0
    for c in cases:
        assert c["states"].shape[1] == po.SWEEP_W
        k = (c["p"] - 0.5) * 2.0 ** 40
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 3
        want = po.states_filter(c["states"], c["p"], c["chr_pos"], 0.5)[0]
        for i, (s, e) in enumerate(c["main"]):
            assert (c["states"][i, s:e] != 0).all() and (want[i, s:e] != 0).all() == (k[i, s:e].sum() <= 0)
            goes += int(want[i, s] == 0)
            stays += int(want[i, s] != 0)
    print(f"{neighbourhood}: {rows} rows, the run goes in {goes} and stays in {stays}")
    assert rows in (171, 153) and goes >= rows // 4 and stays >= rows // 4
    for variant in ("drop_first", "drop_first_sum", "drop_64", "drop_64_sum"):
        changed = sum(_rows_changed(c, variant) for c in cases)
        print(f"{neighbourhood}: {variant} changes {changed} of {rows} rows")
        assert 5 * changed >= rows, (neighbourhood, variant, changed, rows)


def test_half_integer_posteriors_tell_half_even_from_half_up():
    c = po.half_integer_case()
    scaled = c["p"] * po.TWO40
    assert np.array_equal(scaled - np.floor(scaled), np.full(scaled.shape, 0.5))
    want, _, removed = po.states_filter(c["states"], c["p"], c["chr_pos"], 0.5)
    up, _, removed_up = po.states_filter(c["states"], c["p"], c["chr_pos"], 0.5, "half_up")
    assert removed.tolist() == [0, 0, 7] and removed_up.tolist() == [7, 0, 7]
    assert np.array_equal(want[0], c["states"][0]) and not up[0].any()


def test_sums_above_2_to_53_tell_the_rounded_conversion_from_others():
    c = po.big_sum_case()
    wrong = {"truncate": 0, "float_sum": 0}
    for i, ((s, e), mean) in enumerate(zip(po.BIG_RUNS, c["means"])):
        assert e - s >= 16385
        total = sum(np.rint(c["p"][i, s:e] * po.TWO40).astype(np.int64).tolist())
        assert total > 2 ** 53 and total % 4 == i + 1 and float(total) != total
        for thr, stays in ((mean, True), (float(np.nextafter(mean, 0.0)), False)):
            got = po.states_filter(c["states"], c["p"], c["chr_pos"], thr)[0]
            assert bool(got[i, s:e].all()) == stays and (stays or not got[i].any())
            for variant in wrong:
                other = po.states_filter(c["states"], c["p"], c["chr_pos"], thr, variant)[0]
                wrong[variant] += int(not np.array_equal(other[i], got[i]))
    print(f"verdicts of 6 that the deviating conversions get wrong: {wrong}")
    assert wrong["truncate"] >= 1 and wrong["float_sum"] >= 1


def test_own_mean_thresholds_keep_at_and_above_the_mean_and_drop_below():
    cases = po.own_mean_cases()
    lengths = sorted(int((c["states"] != 0).sum()) for c in cases)
    assert len(cases) == 50 and lengths[0] == 1 and lengths[-1] == 130 and {63, 64, 65} <= set(lengths)
    for c in cases:
        below, mean, above = c["thresholds"]
        assert below < mean < above
        removed = [int(po.states_filter(c["states"], c["p"], c["chr_pos"], t)[2][0]) for t in c["thresholds"]]
        assert removed == [1, 0, 0]


@pytest.mark.parametrize("name", list(po.crafted_filter_cases()))
def test_filter_oracle_on_the_crafted_cases(name):
    c = po.crafted_filter_cases()[name]
    got, fraction, removed = po.states_filter(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])
    assert np.array_equal(got, c["want"]) and got.dtype == np.int8
    n_runs = len(po.runs(c["states"][0], so.bounds(c["chr_pos"], c["states"].shape[1])))
    assert removed.tolist() == [n_runs - len(po.runs(got[0], so.bounds(c["chr_pos"], got.shape[1])))]
    assert fraction.tolist() == [float((got != 0).sum()) / got.shape[1]]


def test_the_chain_case_loses_blips_and_keeps_every_long_planted_segment():
    """What tests/test_gpu_states_filter.py relies on, established here without a GPU."""
    c = po.chain_case()
    edges = so.bounds(c["chr_pos"], c["states"].shape[1])
    before = sum(len(po.runs(r, edges)) for r in c["states"])
    after = sum(len(po.runs(r, edges)) for r in c["filtered"])
    total, kept = po.planted_segments_kept(c["truth"], c["filtered"], edges)
    print(f"{before} segments, {after} after the filter, {kept} of {total} planted segments of >= 10 windows kept")
    assert 0 < before - after == int(c["removed"].sum())
    assert total > 1000 and kept == total
    called = c["states"] != 0
    assert np.median(c["neutral"][called]) < 0.5


def test_filter_oracle_refuses_bad_values():
    s = np.array([[0, 1, 1]], dtype=np.int8)
    for bad in (1.5, np.nan, -0.25, np.inf):
        with pytest.raises(ValueError, match="posterior"):
            po.states_filter(s, np.array([[0.1, bad, 0.1]]), {"a": 0})
    with pytest.raises(ValueError, match="call"):
        po.states_filter(np.array([[0, 2, 1]], dtype=np.int8), np.full((1, 3), 0.5), {"a": 0})


# ---- the functions, as far as they go without a GPU -------------------------------------------------------------------------
def _adata(n=4, w=10, chr_pos=None, x=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def test_posteriors_missing_keys_and_bad_arguments():
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(KeyError, match="X_other"):
        cnv.tl.cnv_posteriors(ad, use_rep="other")
    for kw, match in (({"amplitude": 0.0}, "amplitude"), ({"sigma": -1.0}, "sigma"), ({"sigma": np.nan}, "sigma"),
                      ({"switch_prob": 0.0}, "switch_prob"), ({"switch_prob": 1.0}, "switch_prob"),
                      ({"switch_prob": True}, "switch_prob"), ({"switch_prob": 1e-320}, "too close")):
        with pytest.raises(ValueError, match=match):
            cnv.tl.cnv_posteriors(ad, **kw)
    with pytest.raises(ValueError, match="outside"):
        cnv.tl.cnv_posteriors(_adata(chr_pos={"chr1": 0, "chr2": 10}))
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match="chr_pos"):
        cnv.tl.cnv_posteriors(ad)


def test_posterior_window_cap_is_the_headers_and_is_enforced():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    cap = int(re.search(r"#define\s+ICV_POSTERIOR_MAX_WINDOWS\s+(\d+)", header).group(1))
    assert cap == _lib.ICV_POSTERIOR_MAX_WINDOWS == po.MAX_WINDOWS
    assert cap >= 4096 and 32 * cap <= 160 * 1024  # 32 bytes of LDS per window, one cell inside a CU's LDS
    assert int(re.search(r"#define\s+ICV_FILTER_MAX_WINDOWS\s+(\d+)", header).group(1)) == _lib.ICV_FILTER_MAX_WINDOWS
    assert _lib.ICV_FILTER_MAX_WINDOWS * 2 ** 40 < 2 ** 63
    ad = _adata(n=1, x=sp.csr_matrix((1, cap + 1)), chr_pos={"chr1": 0})
    with pytest.raises(ValueError, match=str(cap)):
        cnv.tl.cnv_posteriors(ad)


def test_filter_missing_keys_and_bad_arguments():
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(KeyError, match="X_cnv_states"):
        cnv.tl.cnv_states_filter(ad)
    ad.obsm["X_cnv_states"] = np.zeros((4, 10), dtype=np.int8)
    with pytest.raises(KeyError, match="X_cnv_posterior_neutral"):
        cnv.tl.cnv_states_filter(ad)
    ad.obsm["X_cnv_posterior_neutral"] = np.ones((4, 10))
    for bad in (-0.1, 1.1, np.nan, np.inf, "x", True):
        with pytest.raises(ValueError, match="max_p_normal"):
            cnv.tl.cnv_states_filter(ad, max_p_normal=bad)
    ad.obsm["X_cnv_posterior_neutral"] = np.ones((4, 10), dtype=np.float32)
    with pytest.raises(ValueError, match="float64"):
        cnv.tl.cnv_states_filter(ad)
    ad.obsm["X_cnv_posterior_neutral"] = np.ones((4, 9))
    with pytest.raises(ValueError, match="shape"):
        cnv.tl.cnv_states_filter(ad)
    ad.obsm["X_cnv_states"] = np.zeros((4, 10), dtype=np.int32)
    with pytest.raises(ValueError, match="int8"):
        cnv.tl.cnv_states_filter(ad)


def test_symbols_are_exported_and_declared():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_posterior_chains", "icv_states_filter"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert "cnv_posteriors" in cnv.tl.__all__ and "cnv_states_filter" in cnv.tl.__all__


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes

    from infercnvpy_amd import _lib

    lib = _lib.load()
    m = _lib.Matrix(format=_lib.ICV_CSR, dtype=_lib.ICV_F64, n_rows=0, n_cols=8, ld=8)
    one = ctypes.c_void_p(16)  # never dereferenced: every call below fails in the argument checks (or has no rows)
    ok = dict(amplitude=1.0, h=2.0, ps=0.999, pw=0.0005)

    def chains(mat, n_chr=1, neutral=one, loss=None, gain=None, **kw):
        a = dict(ok, **kw)
        return lib.icv_posterior_chains(ctypes.byref(mat), one, n_chr, a["amplitude"], a["h"], a["ps"], a["pw"], neutral,
                                        loss, gain, None)

    m.indptr = 16
    assert chains(m) == _lib.ICV_OK  # no rows: nothing is launched
    assert chains(m, n_chr=0) == _lib.ICV_ERR_INVALID
    assert chains(m, n_chr=9) == _lib.ICV_ERR_INVALID
    assert chains(m, neutral=None) == _lib.ICV_ERR_INVALID
    assert chains(m, loss=one) == _lib.ICV_ERR_INVALID  # loss without gain
    for kw in ({"amplitude": 0.0}, {"h": math.inf}, {"pw": 1e-320}, {"pw": 0.0}, {"ps": 1.0}, {"ps": math.nan}):
        assert chains(m, **kw) == _lib.ICV_ERR_INVALID, kw
    wide = _lib.Matrix(format=_lib.ICV_CSR, dtype=_lib.ICV_F64, n_rows=0, n_cols=_lib.ICV_POSTERIOR_MAX_WINDOWS + 1, ld=0)
    wide.indptr = 16
    assert chains(wide) == _lib.ICV_ERR_INVALID
    assert str(_lib.ICV_POSTERIOR_MAX_WINDOWS) in lib.icv_last_error().decode()

    def filt(n_rows=0, n_cols=8, n_chr=1, thr=0.5, states=one, p=one, out=one):
        return lib.icv_states_filter(states, p, n_rows, n_cols, one, n_chr, thr, out, one, one, one, None)

    assert filt(n_cols=0) == _lib.ICV_ERR_INVALID
    assert filt(n_chr=0) == _lib.ICV_ERR_INVALID
    assert filt(p=None) == _lib.ICV_ERR_INVALID
    assert filt(out=None) == _lib.ICV_ERR_INVALID
    for thr in (-0.5, 1.5, math.nan):
        assert filt(thr=thr) == _lib.ICV_ERR_INVALID
    assert filt(n_cols=_lib.ICV_FILTER_MAX_WINDOWS + 1) == _lib.ICV_ERR_UNSUPPORTED

"""The oracle of tl.cnv_copy_states (tests/_copy_states_oracle.py) against the three-state oracle, against
exhaustive enumeration and on the planted multi-level case; the header, the library and the argument validation of the
C ABI and of the public function -- none of it needs a GPU."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _copy_states_oracle as co
import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "rounding_ties", "planted777", "full_and_empty"])
def test_three_levels_are_the_three_state_oracle_byte_for_byte(name):
    c = so.case(name)
    a, sigma = c["params"]["amplitude"], c["params"]["sigma"]
    states, sign, fraction, params = co.cnv_copy_states(c["x"], c["chr_pos"], levels=(-a, 0.0, a), sigma=sigma,
                                                        switch_prob=c["params"]["switch_prob"])
    assert states.tobytes() == c["states"].tobytes() and sign.tobytes() == c["states"].tobytes()
    assert fraction.tobytes() == c["fraction"].tobytes()
    assert params["levels"] == [-a, 0.0, a] and params["neutral"] == 1


def test_the_viterbi_path_scores_the_maximum_over_all_paths():
    """K <= 4 states, L <= 5 windows: none of the K^L paths, each summed in rule 3's order, scores higher than the one
    the rules select.  Half the chains have exact emissions (ties between states and between predecessors)."""
    rng = np.random.default_rng(2025)
    tied = 0
    for i in range(240):
        k = int(rng.integers(2, 5))
        z = int(rng.integers(0, k))
        n = int(rng.integers(1, 6))
        if i % 2:
            step = float(rng.uniform(0.1, 0.6))
            mu = [(s - z) * step for s in range(k)]
            h, stay, sw = co.scalars(float(rng.uniform(0.05, 0.4)), float(10.0 ** rng.uniform(-6, -0.4)), k)
            xs = rng.normal(0.0, k * step / 2.0, size=n).tolist()
        else:
            mu = co.every_k_levels(k, z)
            h, stay, sw = co.scalars(0.25, float(rng.choice([1e-3, 0.3, 0.5])), k)
            xs = (rng.integers(-2 * k, 2 * k + 1, size=n) * 0.25).tolist()
        mu, z = co.check_levels(mu)
        got = co.viterbi_chain(xs, mu, z, h, stay, sw)
        scores = [co.path_score(xs, list(p), mu, h, stay, sw) for p in itertools.product(range(k), repeat=n)]
        best = max(scores)
        assert co.path_score(xs, got, mu, h, stay, sw) == best, (xs, mu, got)
        tied += scores.count(best) > 1
    assert tied >= 10  # the chains do produce more than one maximal path


def test_the_end_rule_on_one_window_chromosomes():
    """a = 0.5 and h = 8: every emission is exact.  x = a / 2 ties neutral with +1 and neutral is tried first; 1.5 a ties
    +1 with +2 (and -1.5 a ties -1 with -2) and the state nearer to neutral is tried first; 2.5 a ties +2 with +3."""
    a = 0.5
    mu, z = co.check_levels([k * a for k in co.DEFAULT_STEPS])
    h, stay, sw = co.scalars(0.25, 1e-3, len(mu))
    assert h == 8.0 and co.end_order(6, z) == [2, 1, 3, 0, 4, 5] and co.end_order(4, 0) == [0, 1, 2, 3]
    assert co.end_order(5, 4) == [4, 3, 2, 1, 0]
    for x, want in ((a / 2, 0), (1.5 * a, 1), (-1.5 * a, -1), (2.5 * a, 2), (-a / 2, 0), (0.0, 0), (3.5 * a, 3)):
        e = co.emissions(x, mu, h)
        assert sorted(e)[-1] == sorted(e)[-2] or x in (0.0, 3.5 * a)  # (a tie between the two nearest states)
        assert co.viterbi_chain([x], mu, z, h, stay, sw) == [want + z], x
    x = sp.csr_matrix(np.array([[a / 2, 1.5 * a, -1.5 * a, 2.5 * a]]))
    states, sign, fraction, _ = co.cnv_copy_states(x, {"c1": 0, "c2": 1, "c3": 2, "c4": 3}, levels=mu, sigma=0.25)
    assert states.tolist() == [[0, 1, -1, 2]] and sign.tolist() == [[0, 1, -1, 1]] and fraction.tolist() == [0.75]


def test_planted_levels_six_states_call_what_three_states_cannot():
    """The wrong calls of 3 120, measured with this oracle for the seeds 0-4: six states 15, 22, 16, 25, 21; the
    three-state chain of ``_states_oracle`` with the right single amplitude 505, 511, 518, 538, 509, of which 480 are wrong
    by construction (the windows with |truth| > 1).  Both bounds are conditions on the case."""
    for seed in range(5):
        c = co.case(f"planted_levels_{seed}")
        truth = c["truth"]
        assert truth.shape == (24, 130) and int((truth != 0).sum()) == 1008 and int((np.abs(truth) > 1).sum()) == 480
        wrong6 = int((c["states"] != truth).sum())
        three, _, _ = so.cnv_states(c["x"], c["chr_pos"], amplitude=0.3, sigma=0.1)
        wrong3 = int((three != truth).sum())
        print(f"seed {seed}: wrong calls of {truth.size}: six states {wrong6}, three states {wrong3}")
        assert wrong6 <= co.PLANTED_MOST_WRONG and wrong3 >= co.PLANTED_LEAST_WRONG
        assert np.array_equal(c["sign"], np.sign(c["states"])) and set(np.unique(c["states"])) >= {-1, 0, 1, 2, 3}
        assert np.array_equal(c["fraction"], (c["states"] != 0).sum(axis=1) / 130.0)


@pytest.mark.parametrize("variant", co.VARIANTS)
def test_rounding_case_tells_every_deviating_order_of_operations_from_the_contract(variant):
    """The power of the K = 6 case, measured on the CPU (seed 1, chains of 400 whose calls differ from the contract's, at
    L = 2 / 3 / 6): assoc 10 / 1 / 11, emul 5 / 1 / 8, fma 1 / 1 / 7.  A kernel that evaluates rule 2 or rule 3 in the
    variant's order cannot equal the contract's bytes on this case."""
    c = co.case("rounding_ties")
    assert c["x"].shape[0] == co.ROUNDING_ROWS and len(c["chr_pos"]) == 3 * co.ROUNDING_CHAINS // co.ROUNDING_ROWS > 64
    differ = co.rounding_differences(c, variant)
    print(f"{variant}: chains of {co.ROUNDING_CHAINS} whose calls differ from the contract's: {differ}")
    assert set(differ) == set(co.ROUNDING_LENGTHS) and sum(differ.values()) >= 1
    st = c["states"]
    assert (st[0::2] == 1).mean() > 0.01 and (st[0::2] == 2).mean() > 0.3  # both sides of the tie are called,
    assert (st[1::2] == -1).mean() > 0.01 and (st[1::2] == -2).mean() > 0.3  # and the mirrored rows lose


def test_every_k_cases_reach_every_level():
    for k, z, p in ((6, 2, 1e-3), (6, 2, 0.3), (2, 0, 0.3), (8, 7, 1e-3)):
        c = co.case(f"every_k_{k}_{z}_{p}")
        assert set(np.unique(c["states"])) == set(range(-z, k - z)), (k, z, p)
        assert not c["states"][-1].any() and np.diff(c["x"].indptr)[-1] == 0


# ---- rule 3 in the kernel's O(K) form, and what tells a wrong second best from the contract ---------------------------------------
ALL_K = range(co.MIN_STATES, co.MAX_STATES + 1)
SWITCHES = co.EVERY_K_SWITCH + (co.HIGH_SWITCH,)
TWO_BEST_FLOOR = 5  # chains of a HIGH_SWITCH case that every planted bug changes, at least


@functools.lru_cache(maxsize=None)
def _two_best_case(k, z, p):
    """(every_k(k, z, p), its chains under the contract), computed once for the tests below."""
    c = co.every_k(k, z, p)
    return c, co.contract_chains(c)


def _high_switch_cases(p):
    return [(k, z) + _two_best_case(k, z, p) for k in ALL_K for z in co.high_switch_positions(k)]


@pytest.mark.parametrize("p", SWITCHES)
def test_two_best_form_of_rule_3_gives_the_chains_of_the_contract(p):
    assert co.HIGH_SWITCH > (co.MAX_STATES - 1) / co.MAX_STATES > max(co.EVERY_K_SWITCH)
    for k, z, c, contract in _high_switch_cases(p):
        h, stay, sw = co.scalars(c["kwargs"]["sigma"], p, k)
        assert (sw > stay) == (p == co.HIGH_SWITCH), (k, p)
        assert len(contract) == len(co.chains_of(c)) >= 180 and co.two_best_differences(c, None, contract) == 0, (k, z, p)


@pytest.mark.parametrize("bug", co.TWO_BEST_BUGS)
def test_a_wrong_second_best_is_invisible_while_staying_costs_less_than_leaving(bug):
    """Why the cases at switch_prob 1e-3 and 0.3 cannot see a2 / m2: with stay >= sw state a1 never leaves, and no chain
    of any of them changes under any of the three bugs."""
    for p in co.EVERY_K_SWITCH:
        for k, z, c, contract in _high_switch_cases(p):
            assert co.two_best_differences(c, bug, contract) == 0, (bug, k, z, p)


@pytest.mark.parametrize("bug", co.TWO_BEST_BUGS)
def test_a_wrong_second_best_changes_chains_at_the_high_switch_probability(bug):
    """Chains (of 186 - 222 per case) whose calls a bug changes at switch_prob = 0.999, measured with this restatement, the
    smallest over K and z in {0, K // 2, K - 1}: no_demotion 8 (K = 3, z = 1 and K = 8, z = 0), no_second 10 (K = 7,
    z = 6), first_for_all 42 (K = 2, z = 0).  At K = 2 the loop over r >= 2 is empty: only first_for_all exists there."""
    counts = {}
    for k, z, c, contract in _high_switch_cases(co.HIGH_SWITCH):
        if k == 2 and bug != "first_for_all":
            assert co.two_best_differences(c, bug, contract) == 0
            continue
        counts[(k, z)] = co.two_best_differences(c, bug, contract)
    print(f"{bug}: chains changed per (K, z): {counts}")
    assert len(counts) == (20 if bug == "first_for_all" else 18)
    assert min(counts.values()) >= TWO_BEST_FLOOR, counts


def test_high_switch_cases_are_the_matrices_of_0_3_with_other_calls():
    for k in ALL_K:
        for z in co.high_switch_positions(k):
            high, low = co.case(f"every_k_{k}_{z}_{co.HIGH_SWITCH}"), co.case(f"every_k_{k}_{z}_0.3")
            assert (high["x"] != low["x"]).nnz == 0 and high["params"]["switch_prob"] == co.HIGH_SWITCH
            assert int((high["states"] != low["states"]).sum()) >= 100, (k, z)


def test_three_level_ties_at_switch_0_9_see_a_wrong_second_best():
    """The three-state case of tests/test_gpu_copy_states.py above (K - 1) / K = 2 / 3.  Chains of 270 that change,
    measured: no_demotion 5, no_second 30, first_for_all 71."""
    c = so.ties()
    a, sigma, p = c["kwargs"]["amplitude"], c["kwargs"]["sigma"], 0.9
    h, stay, sw = co.scalars(sigma, p, 3)
    assert sw > stay and co.scalars(sigma, 0.3, 3)[2] < co.scalars(sigma, 0.3, 3)[1]
    three, fraction, _ = so.cnv_states(c["x"], c["chr_pos"], amplitude=a, sigma=sigma, switch_prob=p)
    states, sign, copy_fraction, _ = co.cnv_copy_states(c["x"], c["chr_pos"], levels=(-a, 0.0, a), sigma=sigma, switch_prob=p)
    assert states.tobytes() == three.tobytes() == sign.tobytes() and copy_fraction.tobytes() == fraction.tobytes()
    c["kwargs"] = {"levels": (-a, 0.0, a), "sigma": sigma, "switch_prob": p}
    counts = {bug: co.two_best_differences(c, bug) for bug in (None,) + co.TWO_BEST_BUGS}
    print(f"ties at switch_prob = 0.9: chains of {len(co.chains_of(c))} changed: {counts}")
    assert counts.pop(None) == 0 and min(counts.values()) >= TWO_BEST_FLOOR


# ---- rule 4 by hand, and levels off every lattice ------------------------------------------------------------------------------
@pytest.mark.parametrize("z", range(co.END_RULE_STATES))
def test_end_rule_hand_table_is_what_the_oracle_calls(z):
    c = co.case(f"end_rule_{z}")
    mu, zz = co.check_levels(c["kwargs"]["levels"])
    h = co.scalars(c["kwargs"]["sigma"], c["kwargs"]["switch_prob"], len(mu))[0]
    assert zz == z and h == 8.0 and c["x"].shape == (1, 7) and len(c["chr_pos"]) == 7
    for s, x in enumerate(c["x"].toarray()[0].tolist()):
        e = co.emissions(x, mu, h)
        assert e[s] == e[s + 1] == -0.5 and sorted(e)[-3] < -0.5  # the two nearest states tie exactly
    want = c["want"][0].tolist()
    assert want == [s + 1 - z for s in range(z)] + [s - z for s in range(z, 7)]  # below z the upper state, above the lower
    assert want.count(0) == (1 if z in (0, 7) else 2)  # z wins against both neighbours
    assert c["states"].tobytes() == c["want"].tobytes() and c["sign"].tobytes() == np.sign(c["want"]).tobytes()
    assert c["fraction"].tolist() == [(7 - want.count(0)) / 7.0]


def test_unequal_levels_case_calls_at_least_five_levels():
    c = co.case("unequal_levels")
    mu = c["kwargs"]["levels"]
    steps = np.diff(mu)
    assert len(mu) == 7 and len({round(float(v), 9) for v in steps}) == len(steps)  # no two steps alike
    w = c["x"].shape[1]
    assert c["x"].shape[0] == 14 and w % 4 and w % 64 and 0.5 < c["x"].nnz / (14 * w) < 0.8
    called, counts = np.unique(c["states"], return_counts=True)
    print(f"unequal_levels: calls {dict(zip(called.tolist(), counts.tolist()))}")
    assert len(called) >= 5 and counts.min() >= 20 and (c["states"] != c["sign"]).any()


def test_default_levels_zero_matrix_and_bounds():
    c = so.planted(12, [20, 1, 9], 4)
    states, sign, fraction, params = co.cnv_copy_states(c["x"], c["chr_pos"])
    sigma = so.default_sigma(c["x"])
    assert params["sigma"] == sigma and params["levels"] == [float(k) * (2.0 * sigma) for k in co.DEFAULT_STEPS]
    assert params["neutral"] == 2
    zero = co.cnv_copy_states(sp.csr_matrix((3, 30)), c["chr_pos"])
    assert not zero[0].any() and not zero[1].any() and not zero[2].any() and zero[3]["sigma"] == 0.0
    kw = {"levels": (-0.2, 0.0, 0.2, 0.4), "sigma": 0.1}
    part, _, frac, _ = co.cnv_copy_states(c["x"], None, bounds=[3, 9, 9, 28], **kw)
    assert not part[:, :3].any() and not part[:, 28:].any()
    assert np.array_equal(part[:, 3:9], co.cnv_copy_states(c["x"][:, 3:9], {"c": 0}, **kw)[0])
    assert np.array_equal(frac, (part != 0).sum(axis=1) / 30.0)
    minus = co.cnv_copy_states(c["x"], c["chr_pos"], levels=(-0.2, -0.0, 0.2, 0.4), sigma=0.1)
    assert minus[3]["levels"][1] == 0.0 and np.copysign(1.0, minus[3]["levels"][1]) == 1.0


def test_emission_overflow_is_an_error_and_the_largest_value_below_it_is_not():
    x, pos, kw = so.overflow_case()
    mu = [-0.2, 0.0, 0.2, 0.4]
    with pytest.raises(ValueError, match="overflow"):
        co.cnv_copy_states(x, pos, levels=mu, sigma=kw["sigma"])
    m = co.largest_value_that_does_not_overflow(mu, kw["sigma"])
    assert 1e153 < m < 1e154
    fine = x.copy()
    fine.data[fine.data == 1e160] = m
    assert co.cnv_copy_states(fine, pos, levels=mu, sigma=kw["sigma"])[0].shape == (1, 6)
    fine.data[fine.data == m] = -float(np.nextafter(m, np.inf))
    with pytest.raises(ValueError, match="overflow"):
        co.cnv_copy_states(fine, pos, levels=mu, sigma=kw["sigma"])


# ---- the header, the library and the C ABI -----------------------------------------------------------------------------------
def test_window_cap_is_the_headers_and_symbol_is_exported():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    cap = int(re.search(r"#define\s+ICV_COPY_STATES_MAX_WINDOWS\s+(\d+)", header).group(1))
    assert cap == _lib.ICV_COPY_STATES_MAX_WINDOWS == co.MAX_WINDOWS >= 8192
    assert 10 * cap <= 160 * 1024  # 10 bytes of LDS per window, one cell inside a CU's LDS
    source = open(os.path.join(ROOT, "infercnvpy_amd", "csrc", "icv_copy_states.hpp")).read()
    assert f"kCsMaxWindows = {cap};" in source and "kCsLdsPerWindow = 10;" in source
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    name = "icv_copy_states_viterbi"
    assert name in declared and name in _lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert callable(_engine.copy_states_viterbi)
    assert "cnv_copy_states" in cnv.tl.__all__ and callable(cnv.tl.cnv_copy_states)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    m = _lib.Matrix()
    m.format, m.dtype, m.n_rows, m.n_cols, m.ld = _lib.ICV_DENSE, _lib.ICV_F64, 0, co.MAX_WINDOWS + 1, co.MAX_WINDOWS + 1
    m.values = 8
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first

    def call(levels, neutral, h=8.0, stay=-0.001, sw=-7.6, n_chr=2, n_levels=None, outputs=(one, one, one)):
        mu = (ctypes.c_double * len(levels))(*levels)
        rc = lib.icv_copy_states_viterbi(ctypes.byref(m), one, n_chr, mu, len(levels) if n_levels is None else n_levels,
                                         neutral, h, stay, sw, *outputs, None)
        return rc, lib.icv_last_error().decode()

    good = [-0.5, 0.0, 0.5, 1.0]
    rc, msg = call(good, 1)
    assert rc == _lib.ICV_ERR_INVALID and str(co.MAX_WINDOWS) in msg and "10 bytes" in msg  # n_cols above the cap
    m.n_cols = m.ld = 0
    assert call(good, 1)[0] == _lib.ICV_ERR_INVALID
    m.n_cols = m.ld = 10
    assert call(good, 1)[0] == _lib.ICV_OK  # no rows: nothing runs
    for n_chr in (0, 11):
        assert call(good, 1, n_chr=n_chr)[0] == _lib.ICV_ERR_INVALID
    inf, nan = float("inf"), float("nan")
    bad = [
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
        (dict(levels=good, neutral=1, stay=nan), "stay"),
        (dict(levels=good, neutral=1, sw=-inf), "sw"),
    ]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == _lib.ICV_ERR_INVALID and msg.startswith("copy_states_viterbi: ") and word in msg, (kw, msg)
    for k in range(3):
        outputs = tuple(None if i == k else one for i in range(3))
        assert call(good, 1, outputs=outputs)[0] == _lib.ICV_ERR_INVALID
    assert lib.icv_copy_states_viterbi(ctypes.byref(m), one, 2, None, 4, 1, 8.0, -0.001, -7.6, one, one, one,
                                       None) == _lib.ICV_ERR_INVALID
    assert lib.icv_copy_states_viterbi(None, one, 2, (ctypes.c_double * 4)(*good), 4, 1, 8.0, -0.001, -7.6, one, one, one,
                                       None) == _lib.ICV_ERR_INVALID
    assert call([-0.5, -0.0, 0.5], 1)[0] == _lib.ICV_OK  # -0.0 is a zero
    for k in range(2, 9):
        for z in range(k):
            assert call(co.every_k_levels(k, z), z)[0] == _lib.ICV_OK


# ---- the public function's argument validation ---------------------------------------------------------------------------------
def _adata(n=4, w=10, chr_pos=None, x=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


@pytest.fixture
def no_device(monkeypatch):
    """Every way from the function to the device raises AssertionError: the argument errors must come first."""
    from infercnvpy_amd import _engine

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were refused")

    for name in ("matrix_input", "states_rowsq", "states_absmax", "copy_states_viterbi", "_torch"):
        monkeypatch.setattr(_engine, name, touched)


def test_missing_keys_raise_keyerror_with_the_functions_name(no_device):
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(KeyError, match=r"tl\.cnv_copy_states: X_other not found in adata\.obsm\. Did you run `tl\.infercnv`"):
        cnv.tl.cnv_copy_states(ad, use_rep="other")
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match=r"tl\.cnv_copy_states: chr_pos not found in adata\.uns\['cnv'\]"):
        cnv.tl.cnv_copy_states(ad)
    del ad.uns["cnv"]
    with pytest.raises(KeyError, match="chr_pos"):
        cnv.tl.cnv_copy_states(ad)


def test_window_cap_is_enforced_with_the_message_of_cnv_states(no_device):
    import infercnvpy_amd as cnv

    cap = co.MAX_WINDOWS
    ad = _adata(n=1, x=sp.csr_matrix((1, cap + 1)), chr_pos={"chr1": 0})
    with pytest.raises(ValueError) as err:
        cnv.tl.cnv_copy_states(ad)
    assert str(err.value) == (f"tl.cnv_copy_states: {cap + 1} windows; the kernel keeps a cell's windows in LDS and takes "
                              f"at most {cap}")


@pytest.mark.parametrize("kw, match", [
    ({"levels": (-0.3, 0.0, 0.3), "amplitude": 0.3}, "levels and amplitude"),
    ({"levels": (0.0,)}, "1 states"),
    ({"levels": [0.1 * k for k in range(9)]}, "9 states"),
    ({"levels": ()}, "0 states"),
    ({"levels": (-0.3, 0.0, float("inf"))}, "finite"),
    ({"levels": (float("nan"), 0.0, 0.3)}, "finite"),
    ({"levels": (-0.3, 0.0, 0.3, 0.3)}, "ascend"),
    ({"levels": (0.3, 0.0, -0.3)}, "ascend"),
    ({"levels": (-0.3, 0.1, 0.3)}, "exactly one 0.0"),
    ({"levels": (-0.3, -0.0, 0.0, 0.3)}, "ascend"),  # two zeros cannot ascend
    ({"levels": (0.1, 0.2)}, "exactly one 0.0"),
    ({"levels": "abc"}, "sequence of numbers"),
    ({"levels": 0.3}, "sequence of numbers"),
    ({"amplitude": 0.0}, "amplitude"), ({"amplitude": -1.0}, "amplitude"), ({"amplitude": float("nan")}, "amplitude"),
    ({"amplitude": "big"}, "amplitude"), ({"sigma": 0.0}, "sigma"), ({"sigma": -0.1}, "sigma"),
    ({"sigma": float("inf")}, "sigma"), ({"switch_prob": 0.0}, "switch_prob"), ({"switch_prob": 1.0}, "switch_prob"),
    ({"switch_prob": float("nan")}, "switch_prob"), ({"switch_prob": None}, "switch_prob"),
    ({"switch_prob": 1e-323}, "too close to 0 or 1"),  # p / 2 > 0 and p / 5 == 0
])
def test_bad_parameters_raise_valueerror_before_the_device(no_device, kw, match):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=match) as err:
        cnv.tl.cnv_copy_states(_adata(), **kw)
    assert str(err.value).startswith("tl.cnv_copy_states: ")


@pytest.mark.parametrize("chr_pos, match", [({"chr1": 0, "chr2": 10}, "outside"), ({"chr1": 1, "chr2": 4}, "starts at window 0"),
                                            ({}, "empty")])
def test_bad_chr_pos_raises_before_the_device(no_device, chr_pos, match):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=match):
        cnv.tl.cnv_copy_states(_adata(chr_pos=chr_pos))


def test_check_levels_takes_minus_zero_as_the_neutral_state():
    from infercnvpy_amd.tl._copy_states import check_levels

    mu, z = check_levels((-0.3, -0.0, 0.3, np.float32(0.5)))
    assert z == 1 and mu[1] == 0.0 and np.copysign(1.0, mu[1]) == 1.0 and all(type(v) is float for v in mu)
    assert check_levels([0.0, 1.0]) == ([0.0, 1.0], 0) and check_levels([-1, 0]) == ([-1.0, 0.0], 1)
    assert co.check_levels((-0.3, -0.0, 0.3, 0.5)) == (mu[:3] + [0.5], 1)

"""The oracle of tl.cnv_states (tests/_states_oracle.py) against exhaustive enumeration, its accuracy
on planted segments, and the argument validation of the public function -- none of it needs a GPU."""
import itertools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- rules 3-4 against all 3^T paths ---------------------------------------------------------------------------------------
def _all_scores(xs, a, h, stay, sw):
    """{path: score} of all 3^T state sequences, each summed in the order of rule 3: ((previous + T) + e)."""
    e = [so.emissions(x, a, h) for x in xs]
    tr = [[so.transition(r, s, stay, sw) for s in range(3)] for r in range(3)]
    out = {}
    for path in itertools.product(range(3), repeat=len(xs)):
        sc = e[0][path[0]]
        for t in range(1, len(xs)):
            sc = (sc + tr[path[t - 1]][path[t]]) + e[t][path[t]]
        out[path] = sc
    return out


def _enumerated_choice(xs, a, h, stay, sw):
    """(path that rules 3-4 select, {path: score} of the whole chain), from explicit enumeration only: top[t][s] is the
    largest score over ALL 3^(t + 1) state sequences of the windows 0 .. t that end in s."""
    T = len(xs)
    top, scores = [], None
    for t in range(T):
        scores = _all_scores(xs[:t + 1], a, h, stay, sw)
        top.append([max(v for p, v in scores.items() if p[-1] == s) for s in range(3)])
    best = max(top[T - 1])
    s = next(c for c in so.END_ORDER if top[T - 1][c] == best)  # rule 4
    path = [s]
    for t in range(T - 1, 0, -1):
        cand = {r: top[t - 1][r] + so.transition(r, s, stay, sw) for r in range(3)}
        m = max(cand.values())
        s = next(r for r in [s] + [r for r in range(3) if r != s] if cand[r] == m)  # r = s first, then the lower r
        path.append(s)
    path.reverse()
    return path, scores


def _check_chain(xs, a, h, stay, sw):
    got = so.viterbi_chain(xs, a, h, stay, sw)
    want, scores = _enumerated_choice(xs, a, h, stay, sw)
    best = max(scores.values())
    assert scores[tuple(got)] == so.path_score(xs, got, a, h, stay, sw) == best, (xs, got)
    assert got == want, (xs, got, want)
    return sum(1 for v in scores.values() if v == best)


def test_ties_chains_select_the_ruled_path_among_all_paths():
    c = so.ties()
    dense = c["x"].toarray()
    edges = so.bounds(c["chr_pos"], dense.shape[1])
    kw = c["kwargs"]
    h, stay, sw = so.scalars(kw["sigma"], kw["switch_prob"])
    assert h == 8.0
    seen, tied = set(), 0
    for row in dense:
        for s0, s1 in zip(edges[:-1], edges[1:]):
            xs = tuple(row[s0:s1].tolist())
            assert len(xs) <= 7
            if xs in seen:
                continue
            seen.add(xs)
            tied += _check_chain(list(xs), kw["amplitude"], h, stay, sw) > 1
    assert len(seen) > 100 and tied >= 10  # the case does produce chains with more than one maximal path


def test_random_chains_select_the_ruled_path_among_all_paths():
    rng = np.random.default_rng(2024)
    lattice = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0])
    for i in range(200):
        T = int(rng.integers(1, 8))
        if i % 2:  # generic values and parameters
            sigma = float(rng.uniform(0.05, 0.5))
            a = float(rng.uniform(0.5, 3.0)) * sigma
            p = float(10.0 ** rng.uniform(-6, -0.5))
            xs = rng.normal(0.0, 2.0 * sigma, size=T).tolist()
        else:  # exact emissions: ties between states and between predecessors
            sigma, a, p = 0.25, 0.5, float(rng.choice([1e-3, 0.5, 2.0 / 3.0]))
            xs = lattice[rng.integers(0, len(lattice), size=T)].tolist()
        h, stay, sw = so.scalars(sigma, p)
        _check_chain(xs, a, h, stay, sw)


@pytest.mark.parametrize("variant", so.VARIANTS)
def test_rounding_ties_tell_every_deviating_order_of_operations_from_the_contract(variant):
    """The power of the case, measured on the CPU (seed 1, chains of 400 whose calls differ from the contract's, at
    L = 2 / 3 / 6): assoc 54 / 61 / 92, emul 27 / 79 / 45, fma 67 / 62 / 46.  The bound is a condition on the inputs: a
    kernel that evaluates rule 2 or rule 3 in the variant's order cannot equal the contract's bytes on this case."""
    c = so.case("rounding_ties")
    assert c["x"].shape[0] == so.ROUNDING_ROWS and len(c["chr_pos"]) == 3 * so.ROUNDING_CHAINS // so.ROUNDING_ROWS > 64
    assert all(len(v) == so.ROUNDING_CHAINS for v in c["chains"].values())
    differ = so.rounding_differences(c, variant)
    print(f"{variant}: chains of {so.ROUNDING_CHAINS} whose calls differ from the contract's: {differ}")
    assert set(differ) == set(so.ROUNDING_LENGTHS)
    for L, n in differ.items():
        assert n >= 10, (variant, L, n)


def test_rounding_ties_reach_all_three_calls_and_the_variants_are_valid_chains():
    c = so.case("rounding_ties")
    st = c["states"]
    share = [float((st == v).mean()) for v in (-1, 0, 1)]
    print(f"loss / neutral / gain share of the calls: {share}")
    assert min(share) >= 0.1
    assert (st[0::2] == 1).mean() > 0.3 and (st[1::2] == -1).mean() > 0.3  # the mirrored rows lose where the others gain
    # away from a tie the variants are the contract: they deviate in rounding only
    p = so.planted(12, [20, 1, 9], 4)
    dense = p["x"].toarray()
    h, stay, sw = so.scalars(0.1, 1e-3)
    for row in dense:
        for s0, s1 in ((0, 20), (20, 21), (21, 30)):
            xs = row[s0:s1].tolist()
            want = so.viterbi_chain(xs, 0.2, h, stay, sw)
            assert all(so.viterbi_chain(xs, 0.2, h, stay, sw, v) == want for v in so.VARIANTS)


@pytest.mark.parametrize("w", so.SPLIT_WIDTHS)
def test_output_split_cases_have_calls_at_both_ends_of_every_row_offset(w):
    c = so.case(f"output_split_{w}")
    st = c["states"]
    assert st.shape == (so.SPLIT_ROWS, w)
    offsets = {(i * w) % 4 for i in range(so.SPLIT_ROWS)}
    ends = {(i * w) % 4 for i in range(so.SPLIT_ROWS) if st[i, 0] != 0 and st[i, -1] != 0}
    assert ends == offsets, (w, offsets, ends)
    assert (st != 0).mean() > 0.5


def test_bounds_entry_point_skips_empty_chromosomes_and_leaves_uncovered_windows_neutral():
    c = so.planted(6, [10, 7, 13], 19)
    x, pos = c["x"], c["chr_pos"]
    kw = {"amplitude": 0.2, "sigma": 0.1}
    want = so.cnv_states(x, pos, **kw)
    same = so.cnv_states(x, None, bounds=[0, 10, 17, 30], **kw)
    assert np.array_equal(same[0], want[0]) and np.array_equal(same[1], want[1])
    empty = so.cnv_states(x, None, bounds=[0, 10, 10, 17, 30], **kw)
    assert np.array_equal(empty[0], want[0])
    part, fraction, _ = so.cnv_states(x, None, bounds=[3, 9, 28], **kw)
    assert not part[:, :3].any() and not part[:, 28:].any()
    assert np.array_equal(part[:, 3:9], so.cnv_states(x[:, 3:9], {"c": 0}, **kw)[0])
    assert np.array_equal(part[:, 9:28], so.cnv_states(x[:, 9:28], {"c": 0}, **kw)[0])
    assert np.array_equal(fraction, (part != 0).sum(axis=1) / 30.0)


def test_emission_overflow_is_an_error_and_the_largest_value_below_it_is_not():
    x, pos, kw = so.overflow_case()
    h, stay, sw = so.scalars(kw["sigma"], 1e-3)
    assert so.emissions(1e160, kw["amplitude"], h) == [-np.inf] * 3
    # what rules 1-5 alone make of it: every d is -inf from that window on and the tie rules call the whole row neutral
    assert so.viterbi_chain(x.toarray()[0].tolist(), kw["amplitude"], h, stay, sw) == [1] * 6
    with pytest.raises(ValueError, match="overflow"):
        so.cnv_states(x, pos, **kw)
    with pytest.raises(ValueError, match="overflow"):
        so.cnv_states(-x, pos, **kw)
    m = so.largest_value_that_does_not_overflow(kw["amplitude"], kw["sigma"])
    assert 1e153 < m < 1e154
    fine = x.copy()
    fine.data[fine.data == 1e160] = m
    assert so.cnv_states(fine, pos, **kw)[0].shape == (1, 6)
    fine.data[fine.data == m] = -float(np.nextafter(m, np.inf))
    with pytest.raises(ValueError, match="overflow"):
        so.cnv_states(fine, pos, **kw)


def test_boundaries_and_default_parameters():
    c = so.planted(20, [12, 1, 9], 3)
    x, pos = c["x"], c["chr_pos"]
    st, frac, params = so.cnv_states(x, pos)
    assert params["sigma"] == so.default_sigma(x) and params["amplitude"] == 2.0 * params["sigma"]
    # chains never cross a boundary: every chromosome alone gives the same calls
    kw = {"amplitude": params["amplitude"], "sigma": params["sigma"]}
    for s0, s1 in ((0, 12), (12, 13), (13, 22)):
        part, _, _ = so.cnv_states(x[:, s0:s1], {"c": 0}, **kw)
        assert np.array_equal(part, st[:, s0:s1])
    assert np.array_equal(frac, (st != 0).sum(axis=1) / 22.0)
    # dense, CSC and float32-representable input are the same matrix
    assert np.array_equal(so.cnv_states(x.toarray(), pos)[0], st)
    assert np.array_equal(so.cnv_states(x.tocsc(), pos)[0], st)
    zero = so.cnv_states(sp.csr_matrix((4, 22)), pos)
    assert not zero[0].any() and not zero[1].any() and zero[2]["sigma"] == 0.0


def test_oracle_accuracy_on_planted_segments():
    """Window accuracy of the oracle (default parameters) against the planted truth of planted(200, [40, 1, 25, 60],
    seed), measured on the CPU for seeds 0-4: 0.99130952, 0.99103175, 0.99194444, 0.99337302, 0.99376984.  The bound is
    their minimum rounded down to two decimals: it guards against a later change of the rules, not against noise."""
    for seed in range(5):
        c = so.planted(200, [40, 1, 25, 60], seed)
        st, _, _ = so.cnv_states(c["x"], c["chr_pos"])
        acc = float((st == c["truth"]).mean())
        print(f"seed {seed}: accuracy {acc:.8f}")
        assert acc >= 0.99, (seed, acc)


# ---- the public function's argument validation -----------------------------------------------------------------------------
def _adata(n=4, w=10, chr_pos=None, x=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def test_missing_keys_raise_keyerror():
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(KeyError, match="X_other"):
        cnv.tl.cnv_states(ad, use_rep="other")
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match="chr_pos"):
        cnv.tl.cnv_states(ad)
    del ad.uns["cnv"]
    with pytest.raises(KeyError, match="chr_pos"):
        cnv.tl.cnv_states(ad)


@pytest.mark.parametrize("chr_pos, match", [
    ({"chr1": 0, "chr2": 10}, "outside"),
    ({"chr1": 0, "chr2": -1}, "outside"),
    ({"chr1": 0, "chr2": 4, "chr3": 4}, "same window"),
    ({"chr1": 1, "chr2": 4}, "starts at window 0"),
    ({"chr1": 0, "chr2": 2.5}, "not an integer"),
    ({"chr1": 0, "chr2": "x"}, "not an integer"),
    ({}, "empty"),
    ([0, 4], "must map"),
])
def test_bad_chr_pos_raises_before_any_gpu_work(chr_pos, match):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=match):
        cnv.tl.cnv_states(_adata(chr_pos=chr_pos))


def test_chromosome_bounds_sorts_by_start():
    from infercnvpy_amd.tl._states import chromosome_bounds

    b = chromosome_bounds({"chrX": 7, "chr1": np.int64(0), "chr2": 3}, 9)
    assert b.dtype == np.int32 and b.tolist() == [0, 3, 7, 9]


def test_window_cap_is_the_headers_and_is_enforced():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    cap = int(re.search(r"#define\s+ICV_STATES_MAX_WINDOWS\s+(\d+)", header).group(1))
    assert cap == _lib.ICV_STATES_MAX_WINDOWS == so.MAX_WINDOWS
    assert 9 * cap <= 160 * 1024  # 9 bytes of LDS per window, one cell inside a CU's LDS
    ad = _adata(n=1, x=sp.csr_matrix((1, cap + 1)), chr_pos={"chr1": 0})
    with pytest.raises(ValueError, match=str(cap)):
        cnv.tl.cnv_states(ad)


@pytest.mark.parametrize("kw", [
    {"amplitude": 0.0}, {"amplitude": -1.0}, {"amplitude": float("nan")}, {"amplitude": float("inf")},
    {"amplitude": "big"}, {"sigma": 0.0}, {"sigma": -0.1}, {"sigma": float("inf")}, {"sigma": float("nan")},
    {"switch_prob": 0.0}, {"switch_prob": 1.0}, {"switch_prob": -0.5}, {"switch_prob": 1.5},
    {"switch_prob": float("nan")}, {"switch_prob": None},
])
def test_bad_parameters_raise_valueerror(kw):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=next(iter(kw))):
        cnv.tl.cnv_states(_adata(), **kw)


def test_symbols_are_exported_and_declared():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_states_rowsq", "icv_states_viterbi", "icv_states_fraction"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert "cnv_states" in cnv.tl.__all__


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes

    from infercnvpy_amd import _lib

    lib = _lib.load()
    m = _lib.Matrix()
    m.format, m.dtype, m.n_rows, m.n_cols, m.ld = _lib.ICV_DENSE, _lib.ICV_F64, 0, so.MAX_WINDOWS + 1, so.MAX_WINDOWS + 1
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first
    args = (0.5, 8.0, -0.001, -7.6)
    assert lib.icv_states_viterbi(ctypes.byref(m), one, 1, *args, one, one, None) == _lib.ICV_ERR_INVALID
    assert str(so.MAX_WINDOWS) in lib.icv_last_error().decode()
    m.n_cols = m.ld = 10
    m.values = 8
    assert lib.icv_states_viterbi(ctypes.byref(m), one, 0, *args, one, one, None) == _lib.ICV_ERR_INVALID
    assert lib.icv_states_viterbi(ctypes.byref(m), one, 11, *args, one, one, None) == _lib.ICV_ERR_INVALID
    for bad in ((0.0, 8.0, -0.001, -7.6), (0.5, float("inf"), -0.001, -7.6), (0.5, 0.0, -0.001, -7.6),
                (0.5, 8.0, float("nan"), -7.6), (0.5, 8.0, -0.001, float("-inf"))):
        assert lib.icv_states_viterbi(ctypes.byref(m), one, 2, *bad, one, one, None) == _lib.ICV_ERR_INVALID
    assert lib.icv_states_viterbi(ctypes.byref(m), one, 2, *args, one, one, None) == _lib.ICV_OK  # no rows: nothing runs
    assert lib.icv_states_rowsq(None, one, one, None) == _lib.ICV_ERR_INVALID

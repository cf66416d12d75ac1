"""The oracle of tl.cnv_pseudobulk (tests/_pseudobulk_oracle.py) against Python-int sums and
fractions.Fraction arithmetic, the shift rule, the derivation of the groups, and everything tl.cnv_pseudobulk and its two
entry points refuse before they touch the device.  No GPU."""
import ctypes
import fractions
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _pseudobulk_oracle as pb
import _segments_oracle as sg
import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle against exact arithmetic -----------------------------------------------------------------------------------
def exact_tables(x, rows, group_ptr, shift):
    """S and N with Python ints and Fractions: q is the integer nearest to v 2^e, the even one at a tie."""
    x = sp.csr_matrix(x) if not sp.issparse(x) else x.tocsr()
    n, w = x.shape
    g_count = len(group_ptr) - 1
    S = [[0] * w for _ in range(g_count)]
    N = [[0] * w for _ in range(g_count)]
    for g in range(g_count):
        for r in rows[int(group_ptr[g]):int(group_ptr[g + 1])]:
            if not 0 <= r < n:
                continue
            for c, v in zip(x.indices[x.indptr[r]:x.indptr[r + 1]], x.data[x.indptr[r]:x.indptr[r + 1]]):
                if v == 0:
                    continue
                S[g][int(c)] += round(fractions.Fraction(float(v)) * 2 ** shift)  # (round of a Fraction: ties to even)
                N[g][int(c)] += 1
    return S, N


def edge_inputs():
    """(name, x, codes, n_groups): the edge inputs of the GPU tests, small enough for exact arithmetic."""
    t, b = pb.ties_case(), pb.big_sum_case()
    rng = np.random.default_rng(3)
    codes = rng.integers(-1, 4, size=60)
    codes[codes == 2] = 3  # (group 2 is empty, between two others)
    duplicate = sp.csr_matrix((np.asarray([0.25, 0.5, -0.125, 3.0]), np.asarray([2, 0, 2, 1]), np.asarray([0, 3, 4])),
                              shape=(2, 3))  # unsorted columns, column 2 twice in row 0
    return [
        ("ties", t["x"], t["codes"], 1),
        ("big_sum", b["x"], b["codes"], 1),
        ("sparse_f64", pb.random_sparse(60, 37, 0.3, 1), codes, 4),
        ("sparse_f32", pb.random_sparse(60, 37, 0.3, 2, dtype=np.float32), codes, 4),
        ("dense", pb.random_sparse(60, 5, 0.9, 4).toarray(), codes, 4),
        ("unsorted_duplicate_columns", duplicate, np.asarray([0, 0]), 1),
        ("below_the_limit", np.asarray([[np.nextafter(1024.0, 0.0), -np.nextafter(1024.0, 0.0), 5e-324, 2.0 ** -41]]),
         np.asarray([0]), 1),
    ]


@pytest.mark.parametrize("name, x, codes, n_groups", edge_inputs(), ids=[c[0] for c in edge_inputs()])
def test_sums_are_python_int_sums_and_means_are_fractions_rounded_once(name, x, codes, n_groups):
    got = pb.profiles(x, codes, n_groups)
    shift = got["shift"]
    S, N = exact_tables(x, got["rows"], got["group_ptr"], shift)
    assert got["S"].dtype == np.int64 and got["N"].dtype == np.int32
    assert got["S"].tolist() == S and got["N"].tolist() == N
    for g, L in enumerate(got["n_cells"].tolist()):
        for w in range(got["S"].shape[1]):
            if L == 0:
                assert got["mean"][g, w] == 0.0 and got["fraction"][g, w] == 0.0
                continue
            assert got["mean"][g, w] == pb.exact_mean(S[g][w], L, shift)
            if abs(S[g][w]) <= 2 ** 53:  # (the conversion is exact: the mean is the true quotient rounded once)
                assert got["mean"][g, w] == float(fractions.Fraction(S[g][w], L * 2 ** shift))
            assert got["fraction"][g, w] == float(fractions.Fraction(N[g][w], L))
            assert abs(S[g][w]) < 2 ** 62


def test_ties_go_to_even_and_big_sums_are_exact():
    t = pb.ties_case()
    got = pb.profiles(t["x"], t["codes"], 1)
    assert got["shift"] == 40 and np.array_equal(got["S"][0], t["want_q"])
    assert got["N"][0].tolist() == [1] * t["x"].shape[1]  # (2^-41 rounds to q = 0 and is still a stored value)
    b = pb.big_sum_case()
    got = pb.profiles(b["x"], b["codes"], 1)
    assert got["S"][0].tolist() == b["want_S"]
    naive = b["x"].sum(axis=0) * 2.0 ** 40  # a float64 accumulator
    assert all(int(v) != s for v, s in zip(naive, b["want_S"]))


def test_zeros_are_not_counted():
    x = sp.csr_matrix((np.asarray([0.0, -0.0, 1.5, 0.0]), np.asarray([0, 1, 2, 2]), np.asarray([0, 3, 4])), shape=(2, 3))
    got = pb.profiles(x, np.asarray([0, 0]), 1)
    assert got["N"].tolist() == [[0, 0, 1]] and got["fraction"].tolist() == [[0.0, 0.0, 0.5]]
    assert got["mean"].tolist() == [[0.0, 0.0, 0.75]]


@pytest.mark.parametrize("l_max, shift", [(1, 40), (4095, 40), (4096, 39), (2 ** 20, 31), (10 ** 6, 32)])
def test_the_shift_rule(l_max, shift):
    from infercnvpy_amd.tl import _pseudobulk

    assert pb.shift_of(l_max) == shift == _pseudobulk.profile_shift(l_max)
    # every |q| < 2^(10 + e), so L_max of them stay below 2^62
    assert l_max * 2 ** (10 + shift) <= 2 ** 62
    assert 2.0 ** -(shift + 1) <= (4.6e-13 if l_max <= 4095 else 2.4e-10)


def test_the_planted_clones_are_called_from_the_means_and_not_from_the_votes():
    """The comparison of DESIGN.md 4.17, on the CPU with the oracles: 0 of 810 windows wrong from the clone means, 145
    wrong -- every altered window -- from the vote of the per-cell calls."""
    c = pb.planted_clones()
    chr_pos = so.chr_pos_of(c["lengths"])
    assert int((c["truth"] != 0).sum()) == 145 and c["truth"].size == 810
    means = pb.profiles(c["x"], c["codes"], 3)["mean"]
    calls, _, _ = so.cnv_states(means, chr_pos)
    assert int((calls != c["truth"]).sum()) == 0
    per_cell, _, _ = so.cnv_states(c["x"], chr_pos)
    consensus = sg.group_segments(per_cell, c["codes"], 3, sg.bounds(chr_pos, 270))["consensus"]
    wrong = consensus != c["truth"]
    assert int(wrong.sum()) == 145 and int((wrong & (c["truth"] != 0)).sum()) == 145


# ---- what tl.cnv_pseudobulk refuses before it touches the device ---------------------------------------------------------------
def _adata(n=6, w=10, x=None, chr_pos=None, labels=None):
    from infercnvpy_amd._compat import SimpleAnnData

    labels = list("aabbcc")[:n] if labels is None else labels
    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32), obs=pd.DataFrame({"clone": labels}))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def _no_chr_pos():
    ad = _adata()
    del ad.uns["cnv"]["chr_pos"]
    return ad


BAD = [
    ("missing obsm key", _adata, {"use_rep": "other"}, KeyError,
     "tl.cnv_pseudobulk: X_other not found in adata.obsm. Did you run `tl.infercnv`?"),
    ("missing chr_pos", _no_chr_pos, {}, KeyError,
     "tl.cnv_pseudobulk: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
    ("missing groupby", _adata, {"groupby": "nope"}, KeyError, "tl.cnv_pseudobulk: `nope` not found in `adata.obs`"),
    ("missing cnv_leiden", _adata, {"groupby": "cnv_leiden"}, KeyError,
     "tl.cnv_pseudobulk: `cnv_leiden` not found in `adata.obs`. Did you run `tl.leiden`?"),
    ("1-D X", lambda: _adata(x=np.ones(6)), {}, ValueError, "tl.cnv_pseudobulk: X_cnv must be 2-D"),
    ("empty shape", lambda: _adata(x=np.ones((6, 0))), {}, ValueError, "tl.cnv_pseudobulk: empty matrix of shape (6, 0)"),
    ("min_cells=0", _adata, {"min_cells": 0}, ValueError, "tl.cnv_pseudobulk: min_cells=0 must be an integer >= 1"),
    ("min_cells=True", _adata, {"min_cells": True}, ValueError, "tl.cnv_pseudobulk: min_cells=True must be an integer >= 1"),
    ("min_cells=1.5", _adata, {"min_cells": 1.5}, ValueError, "tl.cnv_pseudobulk: min_cells=1.5 must be an integer >= 1"),
    ("min_cells='x'", _adata, {"min_cells": "x"}, ValueError, "tl.cnv_pseudobulk: min_cells='x' must be an integer >= 1"),
    ("chr_pos outside", lambda: _adata(chr_pos={"chr1": 0, "chr2": 10}), {}, ValueError,
     "tl.cnv_states: chr_pos start 10 is outside [0, 10)"),
    ("chr_pos not at 0", lambda: _adata(chr_pos={"chr1": 1}), {}, ValueError,
     "tl.cnv_states: no chromosome of chr_pos starts at window 0"),
    ("chr_pos empty", lambda: _adata(chr_pos={}), {}, ValueError, "tl.cnv_states: chr_pos is empty"),
    ("every group dropped", _adata, {"min_cells": 3}, ValueError,
     "tl.cnv_pseudobulk: no group of `clone` has min_cells=3 cells"),
]


@pytest.mark.parametrize("cid, make, kw, kind, message", BAD, ids=[c[0] for c in BAD])
def test_every_bad_input_has_its_exception_and_its_whole_message(cid, make, kw, kind, message):
    import infercnvpy_amd as cnv

    kw = {"groupby": "clone", **kw}
    with pytest.raises(kind) as info:
        cnv.tl.cnv_pseudobulk(make(), **kw)
    assert type(info.value) is kind and info.value.args[0] == message


# one input that is wrong in two ways: the keys of obsm, uns and obs, then shape, min_cells, chr_pos, the groups
ORDER = [
    (lambda: _adata(x=np.ones(6)), {"use_rep": "other", "groupby": "nope"}, KeyError, "X_other not found"),
    (_no_chr_pos, {"groupby": "nope"}, KeyError, "chr_pos not found"),
    (lambda: _adata(x=np.ones(6)), {"groupby": "nope"}, KeyError, "`nope` not found"),
    (lambda: _adata(x=np.ones(6)), {"min_cells": 0}, ValueError, "must be 2-D"),
    (lambda: _adata(x=np.ones((6, 0)), chr_pos={}), {"min_cells": 0}, ValueError, "empty matrix"),
    (lambda: _adata(chr_pos={}), {"min_cells": 0}, ValueError, "min_cells=0"),
    (lambda: _adata(chr_pos={}), {"min_cells": 3}, ValueError, "chr_pos is empty"),
]


def test_the_first_fault_in_the_order_of_the_checks_is_the_one_reported():
    import infercnvpy_amd as cnv

    for make, kw, kind, part in ORDER:
        with pytest.raises(kind) as info:
            cnv.tl.cnv_pseudobulk(make(), **{"groupby": "clone", **kw})
        assert part in info.value.args[0], part


# ---- the groups: derived as tl.cnv_segments derives them -----------------------------------------------------------------------
def _groups(labels, min_cells=1):
    from infercnvpy_amd.tl._pseudobulk import group_lists

    kept, n_cells, dropped, rows, group_ptr = group_lists(_adata(n=len(labels), labels=labels), "clone", len(labels), min_cells)
    assert n_cells.dtype == np.int64 and rows.dtype == np.int64 and group_ptr.dtype == np.int64
    return list(kept), n_cells.tolist(), dropped, rows.tolist(), group_ptr.tolist()


def test_group_derivation():
    # categorical with an unused category and a missing label: the categories in their order; the unused one has no
    # cells and is dropped whatever min_cells is
    cat = pd.Categorical(["b", "a", None, "b", "a", "b"], categories=["a", "unused", "b"])
    assert _groups(cat) == (["a", "b"], [2, 3], ["unused"], [1, 4, 0, 3, 5], [0, 2, 5])
    assert _groups(cat, 3) == (["b"], [3], ["a", "unused"], [0, 3, 5], [0, 3])
    # a plain column: order of appearance, the missing label in no group
    plain = np.asarray(["z", "y", None, "z", "x", "z"], dtype=object)
    assert _groups(plain) == (["z", "y", "x"], [3, 1, 1], [], [0, 3, 5, 1, 4], [0, 3, 4, 5])
    assert _groups(plain, 2) == (["z"], [3], ["y", "x"], [0, 3, 5], [0, 3])
    with pytest.raises(ValueError, match="no group of `clone` has min_cells=4 cells"):
        _groups(plain, 4)
    # the same lists as tl.cnv_segments' derivation gives the oracle
    from infercnvpy_amd.tl._groups import group_codes

    codes, groups = group_codes(_adata(n=6, labels=plain), "clone")
    rows, group_ptr = pb.lists(codes, len(groups))
    assert (rows.tolist(), group_ptr.tolist()) == _groups(plain)[3:]
    with pytest.raises(ValueError, match="has 6 labels for the 5 rows"):
        from infercnvpy_amd.tl._pseudobulk import group_lists
        group_lists(_adata(n=6, labels=plain), "clone", 5, 1)


# ---- the library and the package, as far as they go without a GPU -----------------------------------------------------------
def test_symbols_are_exported_and_declared():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_group_profiles", "icv_group_profiles_finish"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert "cnv_pseudobulk" in cnv.tl.__all__ and callable(cnv.tl.cnv_pseudobulk)
    source = open(os.path.join(ROOT, "infercnvpy_amd", "csrc", "icv_pseudobulk.hpp")).read()
    assert f"kPbTile = {pb.TILE};" in source and f"kPbSlab = {pb.SLAB};" in source  # (the sizes the edge cases use)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first
    bad = _lib.ICV_ERR_INVALID
    m = _lib.Matrix()
    m.format, m.dtype, m.n_rows, m.n_cols, m.ld, m.values = _lib.ICV_DENSE, _lib.ICV_F64, 4, 5, 5, 8
    ref = ctypes.byref(m)
    assert lib.icv_group_profiles(None, one, 1, one, 1, 40, one, one, one, None) == bad
    assert lib.icv_group_profiles(ref, None, 1, one, 1, 40, one, one, one, None) == bad
    assert lib.icv_group_profiles(ref, one, 1, None, 1, 40, one, one, one, None) == bad
    assert lib.icv_group_profiles(ref, one, 1, one, 1, 40, None, one, one, None) == bad
    assert lib.icv_group_profiles(ref, one, 1, one, 1, 40, one, None, one, None) == bad
    assert lib.icv_group_profiles(ref, one, 1, one, 1, 40, one, one, None, None) == bad
    assert lib.icv_group_profiles(ref, one, -1, one, 1, 40, one, one, one, None) == bad
    assert lib.icv_group_profiles(ref, one, 1, one, -1, 40, one, one, one, None) == bad
    assert lib.icv_group_profiles(ref, one, 1, one, 1, 41, one, one, one, None) == bad
    assert lib.icv_group_profiles(ref, one, 1, one, 1, -1, one, one, one, None) == bad
    for field, value in (("n_cols", 0), ("n_rows", -1), ("dtype", 7), ("format", 7), ("ld", 4)):
        keep = getattr(m, field)
        setattr(m, field, value)
        assert lib.icv_group_profiles(ref, one, 1, one, 1, 40, one, one, one, None) == bad, field
        setattr(m, field, keep)
    assert b"group_profiles" in lib.icv_last_error()
    fin = lib.icv_group_profiles_finish
    assert fin(None, one, one, 1, 5, 40, one, one, None) == bad
    assert fin(one, None, one, 1, 5, 40, one, one, None) == bad
    assert fin(one, one, None, 1, 5, 40, one, one, None) == bad
    assert fin(one, one, one, 1, 5, 40, None, one, None) == bad
    assert fin(one, one, one, 1, 5, 40, one, None, None) == bad
    assert fin(one, one, one, -1, 5, 40, one, one, None) == bad
    assert fin(one, one, one, 1, 0, 40, one, one, None) == bad
    assert fin(one, one, one, 1, 5, 41, one, one, None) == bad
    assert fin(one, one, one, 1, 5, -1, one, one, None) == bad
    assert fin(None, None, one, 0, 5, 40, None, None, None) == _lib.ICV_OK  # no groups: nothing runs

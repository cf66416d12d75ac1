"""The kernels of tl.cnv_pseudobulk at the smallest shapes at which they can go wrong, through the C ABI and through the
public call, against tests/_pseudobulk_oracle.py: window counts around the tile, group sizes around the slab, CSR rows
around the wavefront, ties of the rounding, sums beyond 2^53, the flags and the magnitude limit."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _pseudobulk_oracle as pb

pytestmark = pytest.mark.gpu

TILE, SLAB = pb.TILE, pb.SLAB
GROUP_SIZES = [1, SLAB - 1, SLAB, 0, SLAB + 1, 2 * SLAB + 1]  # an empty group between two others
N_MISSING = 37


def _matrix(x):
    """The DeviceMatrix of a host matrix as it stands: a CSR's columns are neither sorted nor merged."""
    import torch

    from infercnvpy_amd import _engine

    if sp.issparse(x):
        return _engine.DeviceMatrix(indptr=torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                                    indices=torch.from_numpy(x.indices.astype(np.int32)).cuda(),
                                    data=torch.from_numpy(np.ascontiguousarray(x.data)).cuda(), shape=x.shape, validate=False)
    return _engine.DeviceMatrix(dense=x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda())


def abi(x, rows, group_ptr, shift):
    """(S, N, flags, mean, fraction) of the two entry points as host arrays."""
    import torch

    from infercnvpy_amd import _engine

    total, stored, flags, d_ptr = _engine.group_profiles(_matrix(x), np.asarray(rows, dtype=np.int64),
                                                         np.asarray(group_ptr, dtype=np.int64), shift)
    assert total.dtype == torch.int64 and stored.dtype == torch.int32 and flags.dtype == torch.int32
    mean, fraction = _engine.group_profiles_finish(total, stored, d_ptr, shift)
    assert mean.dtype == torch.float64 and fraction.dtype == torch.float64
    return total.cpu().numpy(), stored.cpu().numpy(), int(flags.item()), mean.cpu().numpy(), fraction.cpu().numpy()


def check_abi(x, rows, group_ptr, shift, label, want_flags=0):
    S, N, flags = pb.tables(x, rows, group_ptr, shift)
    mean, fraction = pb.finish(S, N, group_ptr, shift)
    got = abi(x, rows, group_ptr, shift)
    assert flags == want_flags and got[2] == want_flags, label
    assert np.array_equal(got[0], S) and np.array_equal(got[1], N), label
    assert got[3].tobytes() == mean.tobytes() and got[4].tobytes() == fraction.tobytes(), label
    return S, N, mean, fraction


def _adata(x, labels):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32), obs=pd.DataFrame({"clone": labels}))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0}}
    return ad


def public(x, codes):
    """(mean, fraction) of tl.cnv_pseudobulk for integer codes, -1 a missing label, every code in use."""
    import infercnvpy_amd as cnv

    labels = pd.Categorical.from_codes(codes, categories=[f"g{k}" for k in range(int(codes.max()) + 1)])
    clones = cnv.tl.cnv_pseudobulk(_adata(x, labels), "clone")
    return clones.obsm["X_cnv"], clones.obsm["X_cnv_fraction"]


@functools.lru_cache(maxsize=None)
def shuffled_codes():
    """The groups of GROUP_SIZES interleaved in row order, with missing labels among them."""
    rng = np.random.default_rng(12)
    codes = np.concatenate([np.full(s, g) for g, s in enumerate(GROUP_SIZES)] + [np.full(N_MISSING, -1)])
    rng.shuffle(codes)
    codes.setflags(write=False)
    return codes


# ---- window counts around the tile, group sizes around the slab, every storage --------------------------------------------------
@pytest.mark.parametrize("w", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_window_counts_and_group_sizes(w):
    """Rows of every group span several slabs (2 SLAB + 1 rows: three), W = 2 TILE + 3 takes three tiles; an odd W
    moves the rows of the dense forms through every alignment of a 16-byte load."""
    import torch

    codes = shuffled_codes()
    n = codes.shape[0]
    dense = pb.random_sparse(n, w, 1.0 if w == 1 else 0.03, 100 + w, dtype=np.float32).toarray().astype(np.float64)
    dense[3, :] = np.float32(0.37)  # one full row
    x = sp.csr_matrix(dense)
    rows, group_ptr = pb.lists(codes, len(GROUP_SIZES))
    assert np.diff(group_ptr).tolist() == GROUP_SIZES
    shift = pb.shift_of(max(GROUP_SIZES))
    S, N, mean, fraction = check_abi(x, rows, group_ptr, shift, "csr float64")
    assert (N[5] > 0).any() and not S[3].any() and (mean[3] == 0).all() and (fraction[3] == 0).all()
    forms = {"csr float32": x.astype(np.float32), "dense float64": dense, "dense float32": dense.astype(np.float32)}
    wide = torch.zeros((n, w + 5), dtype=torch.float64, device="cuda")  # a view whose rows are w + 5 apart
    wide[:, 5:] = torch.from_numpy(dense).cuda()
    forms["dense view"] = wide[:, 5:]
    for name, form in forms.items():
        got = abi(form, rows, group_ptr, shift)
        assert got[2] == 0 and np.array_equal(got[0], S) and np.array_equal(got[1], N), name
        assert got[3].tobytes() == mean.tobytes() and got[4].tobytes() == fraction.tobytes(), name
    # the public call leaves the empty group out
    keep = [g for g, s in enumerate(GROUP_SIZES) if s]
    for form in (x, dense.astype(np.float32)):
        got_mean, got_fraction = public(form, np.asarray(codes))
        assert got_mean.tobytes() == mean[keep].tobytes() and got_fraction.tobytes() == fraction[keep].tobytes()


def test_lists_that_overlap_rows_out_of_range_and_groups_without_rows():
    x = pb.random_sparse(50, 70, 0.4, 7)
    rows = np.asarray([4, 9, 4, 49, 0, 9, 9, 12], dtype=np.int64)  # row 4 twice in group 0, row 9 in groups 0, 2 and 3
    group_ptr = np.asarray([0, 4, 4, 6, 8, 8], dtype=np.int64)     # groups 1 and 4 have no rows
    S, N, mean, _ = check_abi(x, rows, group_ptr, 40, "overlap")
    assert np.array_equal(S[3], pb.tables(x, [9, 12], [0, 2], 40)[0][0]) and not S[1].any() and not S[4].any()
    # a row number outside the matrix sets bit 1 and is skipped; the group's length still counts it
    rows_bad = np.asarray([4, 50, 9, -1, 0, 2 ** 40], dtype=np.int64)
    S, N, mean, _ = check_abi(x, rows_bad, [0, 3, 6], 40, "rows out of range", want_flags=2)
    assert np.array_equal(S[0], pb.tables(x, [4, 9], [0, 2], 40)[0][0])
    assert mean[0].tobytes() == ((S[0].astype(np.float64) / 3.0) * 2.0 ** -40).tobytes()
    # no listed rows at all: zeroed tables
    got = abi(x, np.zeros(0, dtype=np.int64), [0, 0, 0], 40)
    assert not got[0].any() and not got[1].any() and got[2] == 0 and not got[3].any() and not got[4].any()


def test_csr_rows_around_the_wavefront():
    """Empty rows, rows of 63, 64 and 65 entries, a full row, unsorted and repeated columns, stored 0.0 and -0.0."""
    rng = np.random.default_rng(21)
    w = 130
    lengths = [0, 63, 64, 65, w, 0, 129, 1, 0]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([rng.permutation(w)[:k] for k in lengths]).astype(np.int32)  # unsorted within a row
    data = rng.normal(0, 2.0, indices.shape[0])
    data[::7] = 0.0
    data[3::7] = -0.0
    indices[indptr[6] + 1] = indices[indptr[6]]  # a column twice in one row
    x = sp.csr_matrix((data, indices, indptr), shape=(len(lengths), w))
    assert not x.has_sorted_indices
    rows, group_ptr = np.arange(len(lengths), dtype=np.int64), [0, 5, 9]
    S, N, _, fraction = check_abi(x, rows, group_ptr, 40, "csr rows")
    assert int(N.sum()) == int((data != 0).sum())  # (stored zeros of either sign are not counted)
    check_abi(x.astype(np.float32), rows, group_ptr, 40, "csr rows float32")
    # the public call, on the canonical form of the same matrix (scipy merges the repeated column by a float add:
    # the oracle reads the merged matrix)
    canon = sp.csr_matrix((data, indices, indptr), shape=x.shape)
    canon.sum_duplicates()
    codes = np.repeat([0, 1], [5, 4])
    want = pb.profiles(canon, codes, 2)
    mean, got_fraction = public(canon, codes)
    assert mean.tobytes() == want["mean"].tobytes() and got_fraction.tobytes() == want["fraction"].tobytes()


def test_ties_go_to_even():
    t = pb.ties_case()
    S, N, _, _ = check_abi(t["x"], [0], [0, 1], 40, "ties dense")
    assert np.array_equal(S[0], t["want_q"]) and (N == 1).all()
    S, _, _, _ = check_abi(sp.csr_matrix(t["x"]), [0], [0, 1], 40, "ties csr")
    assert np.array_equal(S[0], t["want_q"])
    mean, _ = public(t["x"], t["codes"])
    assert mean.tobytes() == (t["want_q"].astype(np.float64) * 2.0 ** -40).tobytes()


def test_sums_beyond_2_to_53_are_exact():
    b = pb.big_sum_case()
    rows, group_ptr = pb.lists(b["codes"], 1)
    for x in (b["x"], sp.csr_matrix(b["x"])):
        S, _, mean, _ = check_abi(x, rows, group_ptr, 40, "big sums")
        assert S[0].tolist() == b["want_S"]
        got, _ = public(x, b["codes"])
        assert got.tobytes() == mean.tobytes()
        assert got[0].tolist() == [pb.exact_mean(s, 64, 40) for s in b["want_S"]]


# ---- the flags and the magnitude limit ----------------------------------------------------------------------------------------
def _one_value(v, kind):
    import torch

    x = np.zeros((5, 9))
    x[1, 2], x[3, 4] = 0.5, v
    return sp.csr_matrix(x) if kind == "csr" else x if kind == "dense" else torch.from_numpy(x).cuda()


@pytest.mark.parametrize("kind", ["csr", "dense", "cuda"])
def test_the_magnitude_limit_and_values_that_are_not_finite(kind):
    import torch

    codes = np.asarray([0, 0, 1, 1, 1])
    below = np.nextafter(1024.0, 0.0)
    for v in (below, -below):
        mean, fraction = public(_one_value(v, kind), codes)
        mean = mean.cpu().numpy() if torch.is_tensor(mean) else mean
        assert mean[1, 4] == pb.exact_mean(int(np.rint(v * 2.0 ** 40)), 3, 40) and mean[0, 2] == 0.25
    for v in (1024.0, -1024.0, 1e300):
        with pytest.raises(ValueError, match="magnitude"):
            public(_one_value(v, kind), codes)
    for v in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="non-finite"):
            public(_one_value(v, kind), codes)
        assert abi(_one_value(v, "dense" if kind == "cuda" else kind), [0, 1, 2, 3, 4], [0, 2, 5], 40)[2] == 1
    # a value that is not finite in a row no list names is not read
    assert abi(_one_value(float("nan"), "csr"), [0, 1, 2, 4], [0, 2, 4], 40)[2] == 0


def test_a_packed_csr_with_a_large_value_in_its_unused_tail():
    import torch

    import infercnvpy_amd as cnv

    x = pb.random_sparse(40, 33, 0.3, 5)
    codes = np.arange(40) % 3
    want = pb.profiles(x, codes, 3)
    for tail in (5000.0, float("nan")):
        data = np.concatenate([x.data, [tail, 1.0, -tail]])
        indices = np.concatenate([x.indices, [0, 1, 2]]).astype(np.int32)
        packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), torch.from_numpy(indices).cuda(),
                               torch.from_numpy(data).cuda(), 33)
        mean, fraction = public(packed, codes)
        assert mean.is_cuda and mean.cpu().numpy().tobytes() == want["mean"].tobytes()
        assert fraction.cpu().numpy().tobytes() == want["fraction"].tobytes()
    # among the stored entries the same value is refused
    data = x.data.copy()
    data[7] = 5000.0
    packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), torch.from_numpy(x.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(np.concatenate([data, [1.0]])).cuda(), 33)
    with pytest.raises(ValueError, match="magnitude 5000.0"):
        public(packed, codes)

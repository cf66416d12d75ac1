"""tl.cnv_changepoints on the GPU at the limits of k_changepoint_levels (csrc/icv_changepoint.hpp), on the bytes of the
oracle (tests/_changepoint_oracle.py): exact ties in chromosomes where a lane has several candidates and the candidates
lie in every row of 16 lanes, constant rows whose costs round below 0.0, a unique minimum in each of the 64 lanes and in
three rounds of candidates, values at the bound of what rule 7 accepts, and a device CSR whose rows are not sorted.
tests/test_changepoint_oracle.py shows on the host which mistake of the kernel each case would expose."""
import functools

import numpy as np
import pytest

import _changepoint_oracle as co
from test_gpu_changepoints import _adata, assert_equal

pytestmark = pytest.mark.gpu

SHUFFLED = ("mixed_n3", "ties_long")


def _run(x, c):
    import infercnvpy_amd as cnv

    return cnv.tl.cnv_changepoints(_adata(x, c["chr_pos"]), inplace=False, return_info=True, **c["kwargs"])


# ---- the bytes, as dense float64 and as CSR --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["csr", "dense"])
@pytest.mark.parametrize("name", co.EDGE_CASES)
def test_the_limit_cases_are_the_oracles_bytes(name, kind):
    c = co.expected(name)
    want = c["want"]
    levels, starts, info = _run(c["x"] if kind == "csr" else c["x"].toarray(), c)
    assert info["sigma"] == want["sigma"] and info["beta"] == want["beta"]
    assert_equal(levels, starts, want, (name, kind))
    if name == "minimum_in_every_lane":  # row r - 1 has its one breakpoint at window r: candidate k = r, lane r % 64
        for r in range(1, co.EVERY_LANE_WINDOWS):
            assert np.flatnonzero(starts[r - 1]).tolist() == [0, r], f"lane {r % co.LANES}, round {r // co.LANES} of k"
    if name == "values_at_the_refusal_bound":
        assert np.isfinite(levels).all()


def test_ties_long_with_stored_zeros_of_both_signs():
    c = co.expected("ties_long")
    dense = c["x"].toarray()
    filler = np.where(np.arange(dense.size) % 2 == 0, -0.0, 0.0).reshape(dense.shape)
    given = np.where(dense == 0, filler, dense)
    assert np.signbit(given[dense == 0]).any() and (given == dense).all()
    levels, starts, _ = _run(given, c)
    assert_equal(levels, starts, c["want"], "dense_with_minus_zeros")


def test_a_value_past_the_refusal_bound_is_refused():
    import infercnvpy_amd as cnv

    c = co.expected("values_at_the_refusal_bound")
    x = c["x"].toarray()
    x[0, 0] = 3e152
    with pytest.raises(ValueError, match="^tl.cnv_changepoints: the value of magnitude 3e\\+152 in X_cnv overflows float64"):
        cnv.tl.cnv_changepoints(_adata(x, c["chr_pos"]), **c["kwargs"])


# ---- a device CSR whose rows hold their entries in any order ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shuffled(name):
    """(PackedCsr with every row's entries permuted, the same matrix as a canonical PackedCsr)."""
    import torch

    import infercnvpy_amd as cnv

    x = co.expected(name)["x"]
    out = []
    for indptr, indices, data in (co.shuffled_rows(x, seed=5), (x.indptr.astype(np.int64), x.indices.astype(np.int32), x.data)):
        out.append(cnv.PackedCsr(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(),
                                 torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64)).cuda(), x.shape[1]))
    return tuple(out)


@pytest.mark.parametrize("name", SHUFFLED)
def test_unsorted_rows_of_a_device_csr_give_the_same_bytes(name):
    c = co.expected(name)
    want = c["want"]
    for what, given in zip(("shuffled", "canonical"), _shuffled(name)):
        levels, starts, info = _run(given, c)
        assert levels.is_cuda and starts.is_cuda
        assert info["sigma"] == want["sigma"] and info["beta"] == want["beta"], what  # (the default sigma reads the rows too)
        assert_equal(levels.cpu().numpy(), starts.cpu().numpy(), want, (name, what))


@pytest.mark.parametrize("name", SHUFFLED)
def test_unsorted_rows_give_the_same_sums_of_squared_differences(name):
    from infercnvpy_amd import _engine

    c = co.expected(name)
    edges = co.bounds(c["chr_pos"], c["x"].shape[1])
    want = np.asarray(co.diffsq(co.rows_of(c["x"]), edges))
    assert (want > 0).any()
    for what, given in zip(("shuffled", "canonical"), _shuffled(name)):
        got = _engine.changepoint_diffsq(_engine.matrix_input(given, "test"), np.asarray(edges, dtype=np.int32)).cpu().numpy()
        assert co.same_bytes(got, want), (name, what)

"""The Ward linkage kernels (``icv_ward_linkage``: icv_ward.hpp, icv_ward_strip.hpp, ``ward_finish``) against the numpy
oracle of the rounds (tests/_ward_oracle.py, checked on the CPU by tests/test_ward_oracle.py).

The linkage matrix and the round count are a pure function of the float32 squared-distance matrix (DESIGN.md
section 5), so every comparison here is an equality: ``assert_array_equal`` on all four columns of Z, ``==`` on the
rounds.  No tolerances.  Every case runs in the three column layouts: spare columns ("strip"), the same buffer with
``ICV_WARD_IN_PLACE=1``, and a row stride of n rounded up to 4 without spare columns."""
import functools

import numpy as np
import pytest

import _ward_cases as W
from _ward_oracle import ward_rounds

pytestmark = pytest.mark.gpu

LAYOUTS = ("spare", "in_place", "plain")
SIZES = [2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 2500, 6000]


def _knobs():
    from infercnvpy_amd import _lib

    _lib.load().icv_developer_knobs_reload()


def _buffer(n, layout):
    """An uninitialised n x n device view with the layout's row stride, and the ``spare`` flag that goes with it."""
    import torch

    from infercnvpy_amd import _engine

    ld = (n + 3) // 4 * 4 if layout == "plain" else _engine.spare_stride(n)
    return torch.empty((n, ld), dtype=torch.float32, device="cuda")[:, :n], layout != "plain"


def _run(layout, monkeypatch, fill, n, compact_x=None):
    """``_engine.ward_linkage`` in one layout on a matrix that ``fill(view)`` writes (the rounds overwrite it).  The
    developer knobs are restored before returning."""
    from infercnvpy_amd import _engine

    try:
        if layout == "in_place":
            monkeypatch.setenv("ICV_WARD_IN_PLACE", "1")
        if compact_x is not None:
            monkeypatch.setenv("ICV_WARD_COMPACT_X", str(compact_x))
        _knobs()
        d2, spare = _buffer(n, layout)
        fill(d2)
        return _engine.ward_linkage(d2, spare=spare)
    finally:
        monkeypatch.delenv("ICV_WARD_IN_PLACE", raising=False)
        monkeypatch.delenv("ICV_WARD_COMPACT_X", raising=False)
        _knobs()


def _run_matrix(layout, monkeypatch, D, **kw):
    import torch

    host = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32))
    return _run(layout, monkeypatch, lambda d2: d2.copy_(host), D.shape[0], **kw)


@functools.lru_cache(maxsize=2)
def _expected(kind, n):
    return ward_rounds(W.tie_matrix(kind, n))


# ---------------------------------------------------------------------------------------------------------------- #
# Ward alone, on matrices written by the test
# ---------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("kind,n,layout", [(k, n, l) for k in W.TIE_KINDS for n in SIZES for l in LAYOUTS])
def test_ward_rounds_equal_oracle_on_tied_matrices(kind, n, layout, monkeypatch):
    """Exact integer distances with duplicates, an all-equal matrix (a chain of n - 1 rounds in which every row is
    searched again), a regular 2-D grid, two- and three-valued matrices: ties in every search, parents at the
    height of their children.  n = 6000 in the spare layout passes the compaction threshold (width > 4096)."""
    Z, rounds = _run_matrix(layout, monkeypatch, W.tie_matrix(kind, n))
    Ze, re_ = _expected(kind, n)
    assert rounds == re_
    np.testing.assert_array_equal(Z, Ze)


@pytest.mark.parametrize("kind", ["int", "three", "grid"])
def test_ward_rounds_equal_oracle_when_compaction_follows_every_round(kind, monkeypatch):
    """ICV_WARD_COMPACT_X=1.05: the spare layout compacts its columns after nearly every round (position maps and
    cached neighbours have to survive it)."""
    n = 6000
    Z, rounds = _run_matrix("spare", monkeypatch, W.tie_matrix(kind, n), compact_x=1.05)
    Ze, re_ = _expected(kind, n)
    assert rounds == re_
    np.testing.assert_array_equal(Z, Ze)


# ---------------------------------------------------------------------------------------------------------------- #
# Ward behind the real Gram: the oracle runs on the GPU's own distance matrix, so any data is exact
# ---------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,d,k", [(2, 4, 1), (3, 2, 1), (10, 3, 2), (257, 20, 6), (1000, 1, 3), (1500, 2, 4),
                                   (1000, 50, 8), (3000, 300, 12), (6000, 48, 9)])
def test_ward_rounds_equal_oracle_behind_the_gram(n, d, k, monkeypatch):
    """``_blobs`` inputs, d = 1 and d = 2 included (where the Gram's float32 error reorders the bottom of scipy's
    tree): the rounding of the distances is separated from the rounds."""
    import torch

    from infercnvpy_amd import _engine
    from test_gpu_parity import _blobs

    xd = torch.from_numpy(_blobs(n, d, k, seed=100 + n)).cuda()
    host = _engine.pairwise_sqeuclidean(xd).cpu().numpy()
    Ze, re_ = ward_rounds(host)
    runs = [(layout, None) for layout in LAYOUTS] + ([("spare", 1.05)] if n == 6000 else [])
    for layout, cx in runs:
        Z, rounds = _run(layout, monkeypatch, lambda d2: _engine.pairwise_sqeuclidean(xd, out=d2), n, compact_x=cx)
        assert rounds == re_, (layout, cx)
        np.testing.assert_array_equal(Z, Ze, err_msg=f"{layout} compact_x={cx}")


# ---------------------------------------------------------------------------------------------------------------- #
# public API on exact inputs: Gram -> rounds -> finish carries no error at all
# ---------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,d,lim", [(2, 3, 2), (3, 3, 2), (65, 3, 2), (257, 17, 7), (1025, 3, 2), (2500, 40, 7),
                                     (2500, 3, 2)])
def test_public_ward_linkage_exact_on_integer_points(n, d, lim):
    import infercnvpy_amd as cnv

    X, D = W.int_points(n, d=d, lim=lim)
    Z, rounds = cnv.tl.ward_linkage(X, return_rounds=True)
    Ze, re_ = ward_rounds(D)
    assert rounds == re_
    np.testing.assert_array_equal(Z, Ze)


# ---------------------------------------------------------------------------------------------------------------- #
# no finite distance: the documented error, not a read before the state arrays
# ---------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [5, 300])
def test_ward_all_inf_matrix_is_an_error(n, layout, monkeypatch):
    """A row without a finite distance has no neighbour (nn = -1): the pair kernels must not index with it, every
    row is searched again once, and the second round without a pair raises."""
    with pytest.raises(ValueError, match="distances are not finite"):
        _run_matrix(layout, monkeypatch, W.all_equal(n, np.inf))
    D = W.all_equal(n)
    D[n - 1, :n - 1] = D[:n - 1, n - 1] = np.inf  # one cluster nobody can reach: the others merge first
    with pytest.raises(ValueError, match="distances are not finite"):
        ward_rounds(D)
    with pytest.raises(ValueError, match="distances are not finite"):
        _run_matrix(layout, monkeypatch, D)

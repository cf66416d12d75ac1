"""The validation tl.leiden, tl.umap and tl.tsne share (graph_entry_flags / k_graph_check of csrc/icv_graph.hpp): every
defect of the stored graph is refused by each of the three engine entry points with the whole message it had when each
feature had its own kernel, two defects report the one that is tested first, t-SNE's "above 2" (now a host comparison
of the largest weight) sits exactly at 2.0f, -0.0 is a zero, and a refused call leaves the state as it was.  Every case
is an argument error the library returns; one ring of five 8-cliques (40 vertices) serves them all."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _leiden_oracle as lo  # noqa: E402

pytestmark = pytest.mark.gpu
N = 40
WHO = ("tl.leiden", "tl.umap", "tl.tsne")
RANGE = "the adjacency matrix has a column index out of range"
SORTED = "the rows of the adjacency matrix must be sorted, without duplicates"
FINITE = "the adjacency matrix has non-finite values"
NEGATIVE = "the adjacency matrix has negative values"
DIAGONAL = "the adjacency matrix has stored diagonal entries"
SYMMETRIC = "the adjacency matrix is not symmetric"
ABOVE_2 = "tl.tsne: the adjacency matrix has values above 2 (affinities are at most 2)"
_cache = {}


def _base():
    """(indptr, indices, data) of the graph, every weight 0.5; the defects below work on copies."""
    if "g" not in _cache:
        g = lo.cliques([8] * 5, ring=True)
        assert g.shape == (N, N) and g.has_sorted_indices
        _cache["g"] = (g.indptr.astype(np.int64), g.indices.astype(np.int32), np.full(g.nnz, 0.5, dtype=np.float32))
    return tuple(a.copy() for a in _cache["g"])


def _at(a, i, j):
    row = a[1][a[0][i]:a[0][i + 1]]
    k = int(np.searchsorted(row, j))
    assert row[k] == j
    return int(a[0][i]) + k


def _set(a, i, j, v, mirror=True):
    a[2][_at(a, i, j)] = v
    if mirror:
        a[2][_at(a, j, i)] = v
    return a


def _insert(a, i, j, v):
    at = int(a[0][i]) + int(np.searchsorted(a[1][a[0][i]:a[0][i + 1]], j))
    indptr = a[0].copy()
    indptr[i + 1:] += 1
    return indptr, np.insert(a[1], at, j).astype(np.int32), np.insert(a[2], at, v).astype(np.float32)


def _delete(a, i, j):
    at = _at(a, i, j)
    indptr = a[0].copy()
    indptr[i + 1:] -= 1
    return indptr, np.delete(a[1], at), np.delete(a[2], at)


def _out_of_range(a):
    a[1][a[0][4] - 1] = N  # the last column of row 3
    return a


def _unsorted(a):
    b = int(a[0][5])
    for arr in a[1:]:
        arr[[b, b + 1]] = arr[[b + 1, b]]
    return a


DEFECTS = {  # each in rows of its own, so that two of them meet only in the flags
    "range": _out_of_range,
    "unsorted": _unsorted,
    "duplicate": lambda a: _insert(a, 6, int(a[1][a[0][6]]), 0.5),
    "nan": lambda a: _set(a, 10, 11, np.nan),
    "inf": lambda a: _set(a, 10, 11, np.inf),
    "negative": lambda a: _set(a, 20, 21, -0.5),
    "diagonal": lambda a: _insert(a, 25, 25, 0.5),
    "no mirror": lambda a: _delete(a, 30, 31),
    "other value": lambda a: _set(a, 33, 34, 0.25, mirror=False),
    "above 2": lambda a: _set(a, 12, 13, 3.0),
}


def _state():
    import torch

    if "s" not in _cache:
        rng = np.random.default_rng(0)
        _cache["s"] = [rng.standard_normal((N, 2)).astype(np.float32) for _ in range(3)]
    return [torch.from_numpy(s).cuda() for s in _cache["s"]]


def _run(who, a, state=None):
    """The entry point behind ``who`` on the graph ``a``; what it returns."""
    import torch

    from infercnvpy_amd import _engine

    dev = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a)
    if who == "tl.leiden":
        return _engine.leiden(*dev)
    y, u, g = _state() if state is None else state
    if who == "tl.umap":
        return _engine.umap_epochs(*dev, y, a=1.577, b=0.895, n_epochs=2)  # (epoch 0 moves nothing: one epoch)
    return _engine.tsne_iterations(*dev, y, u, g, iter_begin=0, iter_end=1)


def _refused(who, a, tail):
    import torch

    state = _state()
    before = [s.clone() for s in state]
    with pytest.raises(ValueError) as info:
        _run(who, a, state)
    assert info.value.args[0] == (tail if tail.startswith("tl.") else f"{who}: {tail}"), who
    for s, b in zip(state, before):  # nothing is touched before the validation has passed
        assert torch.equal(s, b), who


def test_the_graph_itself_passes():
    import torch

    labels, info = _run("tl.leiden", _base())
    assert labels.numel() == N and 1 <= info["n_communities"] <= N
    for who in WHO[1:]:
        state = _state()
        before = state[0].clone()
        _run(who, _base(), state)
        assert bool(torch.isfinite(state[0]).all()) and not torch.equal(state[0], before)


@pytest.mark.parametrize("defect, tail", [
    ("range", RANGE), ("unsorted", SORTED), ("duplicate", SORTED), ("nan", FINITE), ("inf", FINITE), ("negative", NEGATIVE),
    ("diagonal", DIAGONAL), ("no mirror", SYMMETRIC), ("other value", SYMMETRIC)])
def test_every_defect_is_refused_by_all_three_with_its_whole_message(defect, tail):
    for who in WHO:
        _refused(who, DEFECTS[defect](_base()), tail)


@pytest.mark.parametrize("first, second, tail", [
    ("range", "nan", RANGE), ("nan", "negative", FINITE), ("negative", "diagonal", NEGATIVE),
    ("diagonal", "no mirror", DIAGONAL)])
def test_two_defects_report_the_one_that_is_tested_first(first, second, tail):
    for who in WHO:
        _refused(who, DEFECTS[second](DEFECTS[first](_base())), tail)
        _refused(who, DEFECTS[first](DEFECTS[second](_base())), tail)


def test_above_2_is_reported_after_every_flag():
    _refused("tl.tsne", DEFECTS["above 2"](_base()), ABOVE_2)
    _refused("tl.tsne", DEFECTS["above 2"](DEFECTS["no mirror"](_base())), SYMMETRIC)
    _refused("tl.tsne", DEFECTS["above 2"](DEFECTS["inf"](_base())), FINITE)
    # a negative value of large magnitude is no value above 2
    _refused("tl.tsne", _set(_base(), 12, 13, -3.0), NEGATIVE)


def test_above_2_starts_right_after_2():
    import torch

    two = np.float32(2.0)
    after = np.nextafter(two, np.float32(3.0))
    assert after > two and after.dtype == np.float32
    state = _state()
    before = state[0].clone()
    _run("tl.tsne", _set(_base(), 12, 13, two), state)
    assert not torch.equal(state[0], before)
    _refused("tl.tsne", _set(_base(), 12, 13, after), ABOVE_2)
    for v in (two, after):
        state = _state()
        _run("tl.umap", _set(_base(), 12, 13, v), state)
        assert bool(torch.isfinite(state[0]).all()) and not torch.equal(state[0], before)


def test_negative_zero_is_a_zero():
    minus, plus = _set(_base(), 12, 13, np.float32(-0.0)), _set(_base(), 12, 13, np.float32(0.0))
    assert np.signbit(minus[2]).sum() == 2 and np.signbit(plus[2]).sum() == 0
    out = []
    for a in (minus, plus):
        state = _state()
        _run("tl.umap", a, state)  # (not refused as negative)
        out.append(state[0].cpu().numpy())
    assert out[0].tobytes() == out[1].tobytes()
    assert out[0].tobytes() != _cache["s"][0].tobytes()
    # the largest weight is not taken from the bits of -0.0 (0x80000000 would order above every weight)
    for a in (minus, plus):
        state = _state()
        _run("tl.tsne", a, state)

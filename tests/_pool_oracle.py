"""The written contract of tl.cnv_pool_neighbors in numpy, on top of tests/_pseudobulk_oracle.py.

  1. values are those of 4.17 rule 1: stored values are used as float64 (a float32 is promoted exactly), an entry that is
     not stored is 0, a stored 0.0 or -0.0 adds nothing.
  2. the neighbourhood of cell i is N(i) = {i} u {indices[e] : indptr[i] <= e < indptr[i + 1]}: an explicit diagonal entry
     does not count i twice, L_i = |N(i)|, an empty graph row gives N(i) = {i}.  Only the structure of the graph counts:
     its values are never read, a stored 0.0 still lists its neighbour, the graph need not be symmetric.
  3. shift e = min(40, 52 - bit_length(max_i L_i)); every stored magnitude is < 2^10.
  4. S[i,w] = the int64 sum over j in N(i) of rint(x[j,w] 2^e), ties to even.
  5. pooled[i,w] = (double(S[i,w]) / double(L_i)) 2^-e; S = 0 gives +0.0.

So pooled = pb.finish(*pb.tables(x, rows, ptr, e)[:2], ptr, e)[0] with rows / ptr listing sorted(N(i)) per cell.  The
kernel's tile is restated here (TILE) because the edge cases are built around it.
"""
import numpy as np
import scipy.sparse as sp

import _pseudobulk_oracle as pb

TILE = 2048            # windows per workgroup (csrc/icv_pool.hpp: kPoolTile)
GRAPH_LONG_ROW = 512   # the longest graph row other kernels of the package stage (csrc/icv_graph.hpp: kGraphLongRow)
MAX_SHIFT = pb.MAX_SHIFT
LIMIT = pb.LIMIT


def structure(graph):
    """(indptr, indices) of a scipy sparse matrix as it stands (explicit zeros are entries) or of an (indptr, indices[,
    data]) tuple of arrays."""
    if sp.issparse(graph):
        g = graph.tocsr()
        return np.asarray(g.indptr, dtype=np.int64), np.asarray(g.indices, dtype=np.int64)
    return np.asarray(graph[0], dtype=np.int64), np.asarray(graph[1], dtype=np.int64)


def neighbourhoods(graph, n):
    """Rule 2: the list of the n sorted int64 arrays N(i)."""
    indptr, indices = structure(graph)
    assert indptr.shape[0] == n + 1
    out = []
    for i in range(n):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert ((cols >= 0) & (cols < n)).all()
        out.append(np.unique(np.concatenate([[i], cols])).astype(np.int64))
    return out


def lists(graph, n):
    """(rows, ptr, n_cells): the neighbourhoods as the group lists of tests/_pseudobulk_oracle.py."""
    hoods = neighbourhoods(graph, n)
    n_cells = np.asarray([h.shape[0] for h in hoods], dtype=np.int32)
    ptr = np.concatenate([[0], np.cumsum(n_cells, dtype=np.int64)]).astype(np.int64)
    return np.concatenate(hoods).astype(np.int64), ptr, n_cells


def pool(x, graph):
    """dict(pooled float64 n x W, n_cells int32 n, shift, largest, S int64 n x W) of rules 1-5 for the matrix ``x`` (scipy
    sparse or dense) and the graph."""
    n = x.shape[0]
    rows, ptr, n_cells = lists(graph, n)
    largest = int(n_cells.max())
    shift = pb.shift_of(largest)
    S, N, flags = pb.tables(x, rows, ptr, shift)
    assert flags == 0
    pooled = pb.finish(S, N, ptr, shift)[0]
    return {"pooled": pooled, "n_cells": n_cells, "shift": shift, "largest": largest, "S": S}


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def graph_of(rows, n, seed=0):
    """The n x n scipy CSR matrix whose row i stores the columns ``rows[i]`` (made ascending and unique) with random
    positive values; every tenth value is an explicit 0.0 (a distance between duplicate cells)."""
    rng = np.random.default_rng(seed)
    cols = [np.unique(np.asarray(r, dtype=np.int64)) for r in rows]
    indptr = np.concatenate([[0], np.cumsum([c.shape[0] for c in cols])]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int32) if indptr[-1] else np.zeros(0, dtype=np.int32)
    data = rng.random(indices.shape[0]) + 0.5
    data[::10] = 0.0
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


def random_graph(n, longest, seed, diagonal_row=None):
    """A non-symmetric graph whose row i lists (i mod (longest + 1)) random other cells; ``diagonal_row`` also lists
    itself."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        others = np.delete(np.arange(n), i)
        rows.append(rng.choice(others, size=i % (longest + 1), replace=False))
    if diagonal_row is not None:
        rows[diagonal_row] = np.concatenate([rows[diagonal_row], [diagonal_row]])
    return graph_of(rows, n, seed)


def edgeless(n):
    return sp.csr_matrix((n, n), dtype=np.float64)


def complete(n):
    return graph_of([np.delete(np.arange(n), i) for i in range(n)], n)


# ---- the case builders shared by the CPU test of this oracle and the GPU tests --------------------------------------------------
def storage_case():
    """n = 37, W = 70: rows of 0 .. 9 graph entries, row 5 with an explicit diagonal entry; float32 numbers with stored
    0.0 / -0.0, so that every storage holds the same values.  dict(x canonical CSR float64, graph)."""
    x = pb.random_sparse(37, 70, 0.3, 21, dtype=np.float32).astype(np.float64)
    graph = random_graph(37, 9, 22, diagonal_row=5)
    assert 5 in graph.indices[graph.indptr[5]:graph.indptr[6]] and (graph.data == 0).any()
    return {"x": x, "graph": graph}


def tile_edges_case(w):
    """n = 9 with values in the last window of every tile, the first window of the next and window w - 1, on a sparse
    background.  dict(x canonical CSR float64 (float32 numbers), graph)."""
    rng = np.random.default_rng(w)
    dense = rng.normal(0.0, 0.5, (9, w)).astype(np.float32).astype(np.float64) * (rng.random((9, w)) < 0.02)
    marks = sorted({c for t in range(TILE, w + 1, TILE) for c in (t - 1, t) if c < w} | {w - 1, 0})
    for k, c in enumerate(marks):
        dense[:, c] = (np.arange(9) - 4.0 + 0.25 * k) * 0.125
    dense[3] = 0.0  # (an empty row among them)
    return {"x": sp.csr_matrix(dense), "graph": random_graph(9, 5, w + 1)}


def graph_rows_case():
    """n = 701, W = 33: row 0 lists all 700 others (longer than GRAPH_LONG_ROW), rows 1 .. 5 have 0, 1, 63, 64 and 65
    entries, row 6 lists only itself, the others 3 each."""
    n = 701
    rng = np.random.default_rng(31)
    rows = [np.delete(np.arange(n), 0)]
    for i, k in zip(range(1, 6), (0, 1, 63, 64, 65)):
        rows.append(rng.choice(np.delete(np.arange(n), i), size=k, replace=False))
    rows.append(np.asarray([6]))
    for i in range(7, n):
        rows.append(rng.choice(np.delete(np.arange(n), i), size=3, replace=False))
    assert len(rows[0]) > GRAPH_LONG_ROW
    return {"x": pb.random_sparse(n, 33, 0.4, 32), "graph": graph_of(rows, n, 33)}


def matrix_rows_case():
    """n = 12, W = 130: rows 0 .. 2 empty, rows 3 .. 5 with 63 / 64 / 65 stored entries, row 6 full (130 stored), the rest
    random; cell 0's neighbourhood is {0, 1, 2}: empty rows only."""
    w = 130
    rng = np.random.default_rng(41)
    dense = np.zeros((12, w))
    for r, k in ((3, 63), (4, 64), (5, 65), (6, w)):
        dense[r, rng.choice(w, size=k, replace=False)] = rng.normal(0.0, 0.5, k)
    dense[7:] = rng.normal(0.0, 0.5, (5, w)) * (rng.random((5, w)) < 0.2)
    dense[dense == 0] = 0.0
    x = sp.csr_matrix(dense)
    assert np.diff(x.indptr)[:7].tolist() == [0, 0, 0, 63, 64, 65, w]
    rows = [[1, 2], [0], [], [4, 5, 6], [3, 6, 11], [0, 6], [1], [3, 4, 5, 6], [0, 1, 2], [10], [6, 9], [7]]
    return {"x": x, "graph": graph_of(rows, 12, 42)}


def hub_case():
    """n = 4 097, W = 5: cell 0 lists the 4 096 others, so L = 4 097 and the shift of every cell drops to 39."""
    n = 4097
    rng = np.random.default_rng(51)
    rows = [np.arange(1, n)] + [[(i * 7) % n] for i in range(1, n)]
    x = rng.normal(0.0, 0.5, (n, 5))
    x[rng.random((n, 5)) < 0.3] = 0.0
    return {"x": sp.csr_matrix(x), "graph": graph_of(rows, n, 52)}


def planted_graph(x, k):
    """The numpy stand-in of tl.pca + pp.neighbors: the projection of the rows of ``x`` onto its top 50 right singular
    vectors (not centred), and per cell the exact k - 1 nearest other cells by Euclidean distance (ties to the lower cell
    number).  A scipy CSR matrix of the distances."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    _, _, vt = np.linalg.svd(x, full_matrices=False)
    y = x @ vt[:50].T
    d2 = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k - 1]
    order.sort(axis=1)
    data = np.sqrt(np.take_along_axis(d2, order, axis=1))
    indptr = np.arange(n + 1, dtype=np.int64) * (k - 1)
    return sp.csr_matrix((data.ravel(), order.ravel().astype(np.int32), indptr), shape=(n, n))


def wrong_calls(states, clone, truth):
    """The number of (cell, window) calls that differ from the planted sign (normal cells, clone -1: all neutral)."""
    want = np.zeros(states.shape, dtype=np.int8)
    tumour = clone >= 0
    want[tumour] = np.sign(truth[clone[tumour]]).astype(np.int8)
    return int((states != want).sum())

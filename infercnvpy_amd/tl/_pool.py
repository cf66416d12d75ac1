"""tl.cnv_pool_neighbors: every cell's CNV profile averaged with those of its graph neighbours (no counterpart in the
reference).

Between the single cell, whose windows are mostly noise, and the clone mean of ``tl.cnv_pseudobulk``, which needs a
clustering and erases everything inside a clone, lies the step that users of inferCNV-style tools take by hand: pool each
cell with its nearest neighbours in CNV space (kNN smoothing, metacells).  Averaging a cell with its 14 neighbours divides
the noise of a window by about the square root of 15, and the result still has one row per cell, so every per-cell
function of this package runs on it unchanged.  The means are those of the written contract of DESIGN.md 4.21: every
stored value is rounded once to a fixed-point int64, the sums are integer sums and one division gives the mean, so the
result is a pure function of (matrix values, graph structure) and equals ``tests/_pool_oracle.py`` bit for bit, whatever
the storage of either.
"""
from __future__ import annotations

import time

import numpy as np

from .. import _engine
from ._graph import _is_tensor, graph_source, resolve_graph
from ._hmm import chromosome_bounds
from ._pseudobulk import MAX_MAGNITUDE, profile_shift

WHO = "tl.cnv_pool_neighbors"


def cnv_pool_neighbors(adata, use_rep="cnv", key_added="cnv_pooled", *, neighbors_key="cnv_neighbors", adjacency=None,
                       obsp=None, inplace=True, return_info=False):
    """Replace every cell's CNV profile by the exact mean over the cell and its neighbours in a graph of cells.

    ``tl.pca(adata); pp.neighbors(adata); tl.cnv_pool_neighbors(adata)`` followed by
    ``tl.cnv_states(adata, use_rep="cnv_pooled")`` calls the alterations of every cell from the mean of the cell and its
    nearest neighbours in CNV space; ``tl.cnv_posteriors``, ``tl.cnv_changepoints``, ``tl.cnv_correlation``,
    ``tl.cnv_pseudobulk`` and ``pl.chromosome_heatmap`` take the same ``use_rep``.  Pooling the result again
    (``use_rep="cnv_pooled", key_added="cnv_pooled2"``) is a second diffusion step.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W) is pooled: a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, float32 or float64.  Stored values are used as float64,
        an entry that is not stored is 0.  ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        The results go to ``obsm[f"X_{key_added}"]``, ``obs[key_added + "_n_cells"]`` and ``uns[key_added]``.
    neighbors_key, adjacency, obsp
        The graph, looked for in this order: ``adjacency``, ``adata.obsp[obsp]``,
        ``adata.obsp[adata.uns[neighbors_key]["distances_key"]]``: the kNN *distances* of ``pp.neighbors``, in which every
        row lists exactly ``n_neighbors - 1`` other cells, so that every cell is averaged over the same number of cells
        (the symmetrised connectivities, with their hubs, work through ``obsp=``).  A scipy sparse matrix or a tuple
        ``(indptr int64, indices int32, data)`` of CUDA tensors with strictly ascending columns in every row.  Only the
        structure is used: the values are never read (a stored 0.0 still lists its neighbour), the graph need not be
        symmetric, a diagonal entry changes nothing, a cell without entries keeps its own profile.
    inplace
        ``False``: return ``(pooled, n_cells)`` and leave ``adata`` as it is.
    return_info
        Also return a dict: ``shift``, ``largest`` (the largest neighbourhood) and ``stage_ms`` (host clocks of the stages
        ``upload``, ``sizes`` and ``pool``; each ends in a copy to the host).

    Returns
    -------
    With ``inplace`` nothing (the info dict when ``return_info``), after storing

    * ``obsm[f"X_{key_added}"]``: n x W float64, the mean over ``N(i) = {i} u {the cells row i of the graph lists}``;
      a numpy array for host input, a CUDA tensor for ``PackedCsr`` / CUDA-tensor input (of the matrix nothing is read
      back then: two pairs of scalars and the n sizes below are),
    * ``obs[key_added + "_n_cells"]``: int32, the size of every neighbourhood,
    * ``uns[key_added]``: ``{"chr_pos": a copy, "params": {"shift", "largest"}, "use_rep", "graph"}`` with ``graph`` the
      key of ``adata.obsp`` that was used or ``"adjacency"``.

    With ``e = shift = min(40, 52 - bit_length(largest))`` every value is rounded once to a multiple of ``2^-e`` and all
    further arithmetic is exact up to the one division: a mean is within ``2^-(e+1)`` of the true mean.  A non-finite value
    raises ``ValueError``, and so does a stored magnitude of 1024 or more.
    """
    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"{WHO}: {key} not found in adata.obsm. Did you run `tl.infercnv`?")
    if use_rep not in adata.uns or "chr_pos" not in adata.uns[use_rep]:
        raise KeyError(f"{WHO}: chr_pos not found in adata.uns['{use_rep}']. Did you run `tl.infercnv`?")
    x = adata.obsm[key]
    shape = getattr(x, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError(f"{WHO}: {key} must be 2-D")
    n, w = int(shape[0]), int(shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"{WHO}: empty matrix of shape {(n, w)}")
    chr_pos = adata.uns[use_rep]["chr_pos"]
    chromosome_bounds(chr_pos, w, WHO)
    source = graph_source(adata, neighbors_key, adjacency, obsp, "distances_key")
    host, dev, n_graph = resolve_graph(WHO, adata, neighbors_key, adjacency, obsp, "distances_key")
    if n_graph != n:
        raise ValueError(f"{WHO}: the graph has {n_graph} vertices, {key} has {n} rows")
    if dev is not None and not (_is_tensor(dev[0]) and dev[0].is_cuda and dev[1].is_cuda
                                and str(dev[0].dtype) == "torch.int64" and str(dev[1].dtype) == "torch.int32"):
        raise ValueError(f"{WHO}: a device graph is (indptr int64, indices int32, data) of CUDA tensors")

    torch = _engine._torch()
    on_device = isinstance(x, (_engine.PackedCsr, torch.Tensor))
    stage_ms = {}
    t0 = time.perf_counter()
    dm = _engine.matrix_input(x, WHO)
    with torch.cuda.device(dm.device):
        free, _total = torch.cuda.mem_get_info()
        if n * w * 8 > free:
            raise ValueError(f"{WHO}: the {n} x {w} float64 result takes {n * w * 8} bytes, {free} are free on the device; "
                             "pool the rows in parts")
        if dev is None:
            g_indptr, g_indices = (torch.from_numpy(a).cuda() for a in host[:2])
            g_data = None
        else:
            g_indptr, g_indices, g_data = (t.to(dm.device) for t in dev)
        g_indptr, g_indices = _engine.neighbor_pool_graph(WHO, g_indptr, g_indices, g_data)
        stage_ms["upload"] = (time.perf_counter() - t0) * 1e3

        # one copy to the host: the largest neighbourhood, which fixes the shift, and what the graph is flagged for
        t0 = time.perf_counter()
        n_cells, flags = _engine.neighbor_pool_sizes(g_indptr, g_indices)
        largest, bits = torch.stack([n_cells.max(), flags[0]]).cpu().tolist()
        stage_ms["sizes"] = (time.perf_counter() - t0) * 1e3
        if bits & _engine.POOL_FLAG_COLUMN:
            raise ValueError(f"{WHO}: the graph has a column outside [0, {n})")
        if bits & _engine.POOL_FLAG_ORDER:
            raise ValueError(f"{WHO}: the columns of every row of the graph must ascend strictly")
        shift = profile_shift(largest)

        # the other one: the flag of a non-finite value and the largest stored magnitude
        t0 = time.perf_counter()
        pooled = _engine.neighbor_pool(dm, g_indptr, g_indices, shift, n_cells, flags)
        absmax = _engine.states_absmax(_engine.states_stored_values(dm))
        bits, m = _engine.flag_and_absmax(flags, absmax)
        if bits & _engine.POOL_FLAG_NONFINITE:
            raise ValueError(f"{WHO}: {key} has non-finite values")
        if not m < MAX_MAGNITUDE and isinstance(x, _engine.PackedCsr):
            # (the m of a PackedCsr covers the unused tail of its buffers: look at the stored entries alone)
            m = float(_engine.states_absmax(x.data[:x.nnz()]).item())
        if not m < MAX_MAGNITUDE:
            raise ValueError(f"{WHO}: {key} has a stored value of magnitude {m!r}; the exact sums take "
                             f"magnitudes below {MAX_MAGNITUDE:g}: rescale the matrix or clip the value")
        sizes = n_cells.cpu().numpy()
        if not on_device:
            pooled = pooled.cpu().numpy()
        stage_ms["pool"] = (time.perf_counter() - t0) * 1e3

    info = {"shift": shift, "largest": int(largest), "stage_ms": stage_ms}
    if not inplace:
        return (pooled, sizes, info) if return_info else (pooled, sizes)
    adata.obsm[f"X_{key_added}"] = pooled
    adata.obs[key_added + "_n_cells"] = sizes
    adata.uns[key_added] = {"chr_pos": dict(chr_pos), "params": {"shift": shift, "largest": int(largest)},
                            "use_rep": use_rep, "graph": source}
    return info if return_info else None

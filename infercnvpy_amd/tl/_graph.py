"""What tl.leiden, tl.umap and tl.tsne share on the host: the intake of the graph, the counter hash behind the initial
positions, the checks whose messages differ only in the function's name, the initial positions and the common tail.
``who`` is that name ("tl.leiden", ...), the prefix of every message."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .. import _engine

_MASK = (1 << 64) - 1


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def graph_source(adata, neighbors_key, adjacency, obsp, which="connectivities_key"):
    """Where the graph comes from: "adjacency", or the key of ``adata.obsp`` (``obsp``, else the one that
    ``adata.uns[neighbors_key][which]`` names).  ``KeyError`` for a key that is not there."""
    if adjacency is not None:
        return "adjacency"
    if obsp is not None:
        if obsp not in adata.obsp:
            raise KeyError(f"{obsp!r} is not in adata.obsp. Did you run `pp.neighbors`?")
        return obsp
    if neighbors_key not in adata.uns:
        raise KeyError(f"{neighbors_key!r} is not in adata.uns. Did you run `pp.neighbors`?")
    key = adata.uns[neighbors_key][which]
    if key not in adata.obsp:
        raise KeyError(f"{key!r} is not in adata.obsp. Did you run `pp.neighbors`?")
    return key


def _graph(adata, neighbors_key, adjacency, obsp, which="connectivities_key"):
    if adjacency is not None:
        return adjacency
    return adata.obsp[graph_source(adata, neighbors_key, adjacency, obsp, which)]


def _host_csr(g, who="tl.leiden"):
    """Canonical CSR arrays (int64, int32, float32 / float64) of a scipy matrix; shape errors before the GPU."""
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise ValueError(f"{who}: the adjacency matrix must be square")
    if g.shape[0] < 1:
        raise ValueError(f"{who}: the adjacency matrix is empty")
    a = sp.csr_matrix(g)
    if a is g:
        a = a.copy()
    a.sum_duplicates()
    a.sort_indices()
    data = a.data if a.data.dtype in (np.float32, np.float64) else a.data.astype(np.float64)
    return a.indptr.astype(np.int64), a.indices.astype(np.int32), np.ascontiguousarray(data)


def resolve_graph(who, adata, neighbors_key, adjacency, obsp, which="connectivities_key"):
    """(host, dev, n): the graph as the host arrays of :func:`_host_csr` (scipy matrix) or as the caller's tuple of CUDA
    tensors (the other one is None), and its number of vertices, which must be ``adata.n_obs``.  ``which``: the entry of
    ``adata.uns[neighbors_key]`` that names the default graph."""
    g = _graph(adata, neighbors_key, adjacency, obsp, which)
    host = dev = None
    if isinstance(g, (tuple, list)) and len(g) == 3 and all(_is_tensor(t) for t in g):
        dev = g
        n = int(g[0].numel()) - 1
        if n < 1:
            raise ValueError(f"{who}: the adjacency matrix is empty")
    elif sp.issparse(g):
        host = _host_csr(g, who)
        n = len(host[0]) - 1
    else:
        raise ValueError(f"{who}: the graph must be a scipy sparse matrix or (indptr, indices, data) CUDA tensors")
    if adata is not None and hasattr(adata, "n_obs") and adata.n_obs != n:
        raise ValueError(f"{who}: the graph has {n} vertices, adata has {adata.n_obs} cells")
    return host, dev, n


def _mix_int(z):
    z &= _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def _uniform24(seed, tag, n, c):
    """n x c float64 numbers in [0, 1): the top 24 bits of mix(mix(seed ^ mix(tag)) ^ (i c + j))."""
    z = np.uint64(_mix_int((seed & _MASK) ^ _mix_int(tag))) ^ np.arange(n * c, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).reshape(n, c)


def check_components(who, n_components):
    if n_components not in (2, 3) or isinstance(n_components, bool):
        raise ValueError(f"{who}: n_components={n_components!r} must be 2 or 3")
    return int(n_components)


def check_seed(who, random_state):
    """The seed of a ``random_state`` that int() accepts (the caller's combined message covers one it does not)."""
    seed = int(random_state)
    if seed != random_state:
        raise ValueError(f"{who}: random_state={random_state!r} is not an integer")
    return seed


def resolve_init(who, adata, init_pos, named, n, c):
    """``init_pos`` as one of the two method names ``named``, or as the given n x c positions (a key of ``adata.obsm``
    is looked up): a CUDA tensor as it is, anything else as a finite host float32 array."""
    init = init_pos
    if isinstance(init, str) and init not in named:
        if adata is None or init not in adata.obsm:
            raise KeyError(f"{who}: init_pos={init!r} is neither {named[0]!r}, {named[1]!r} nor a key of adata.obsm")
        init = adata.obsm[init]
    if not isinstance(init, str):
        if tuple(init.shape) != (n, c):
            raise ValueError(f"{who}: init_pos has shape {tuple(init.shape)}, expected {(n, c)}")
        if not _is_tensor(init):
            init = np.ascontiguousarray(init, dtype=np.float32)
            if not np.isfinite(init).all():
                raise ValueError(f"{who}: init_pos has non-finite values")
    return init


def init_to_device(who, init, device):
    """The float32 device tensor the layout starts from and is updated in: a copy of a given tensor (finite), or the
    upload of a host array."""
    torch = _engine._torch()
    if not _is_tensor(init):
        return torch.from_numpy(init).to(device)
    y = init.detach().to(device=device, dtype=torch.float32).contiguous().clone()
    if not bool(torch.isfinite(y).all().item()):
        raise ValueError(f"{who}: init_pos has non-finite values")
    return y


def finish(adata, slot, key_added, result, params, info, inplace, return_info):
    """Store ``result`` (``slot`` "obs": under ``key_added``; "obsm": under ``X_<key_added>``) and the parameters when
    ``inplace``; what the function returns."""
    if inplace:
        getattr(adata, slot)[key_added if slot == "obs" else f"X_{key_added}"] = result
        adata.uns[key_added] = {"params": params}
        return (result, info) if return_info else None
    return (result, info) if return_info else result

"""Times of tl.cnv_pool_neighbors at the geometry of the tl.cnv_states figures (100 000 cells x 1 802 windows, 13 % stored,
float64 CSR, HBM-resident as tl.infercnv leaves it) with a random 14-regular graph (every row lists 14 distinct other
cells), and for the dense float32 form of the same matrix.

    python tools/time_pool_neighbors.py [--cells 100000] [--windows 1802] [--density 0.13] [--neighbors 14] [--reps 20]

Device-event times (median and minimum over --reps launches after a warm-up), all from one run: icv_neighbor_pool_sizes,
icv_neighbor_pool, the route to the same bytes that the library had before it (icv_group_profiles +
icv_group_profiles_finish with every cell's neighbourhood as a group: two n x W tables in HBM, global integer atomics, a
second pass to divide), icv_states_viterbi on the pooled rows, and a device-to-device copy of the n x W float64 output.
The two routes are compared on the bytes."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--neighbors", type=int, default=14)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine
    from infercnvpy_amd.tl._hmm import chromosome_bounds
    from infercnvpy_amd.tl._pseudobulk import profile_shift

    n, w, k = a.cells, a.windows, a.neighbors
    gen = torch.Generator(device="cuda").manual_seed(0)
    keep = torch.rand((n, w), device="cuda", generator=gen) < a.density
    dense = torch.randn((n, w), device="cuda", generator=gen, dtype=torch.float64) * 0.5 * keep
    indptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    indptr[1:] = keep.sum(dim=1).cumsum(0)
    indices = keep.nonzero()[:, 1].to(torch.int32).contiguous()  # (row-major order: ascending columns in every row)
    packed = cnv.PackedCsr(indptr, indices, dense[keep].contiguous(), w)
    nnz = int(indptr[-1].item())
    dense32 = dense.to(torch.float32)
    del keep, dense

    # every row: k distinct other cells anywhere in the matrix, ascending (offsets 1 .. n - 1 from the cell; a row that drew
    # one twice draws again)
    rng = np.random.default_rng(1)
    cols = np.sort((np.arange(n)[:, None] + rng.integers(1, n, size=(n, k))) % n, axis=1)
    while True:
        again = np.flatnonzero((np.diff(cols, axis=1) == 0).any(axis=1))
        if again.shape[0] == 0:
            break
        cols[again] = np.sort((again[:, None] + rng.integers(1, n, size=(again.shape[0], k))) % n, axis=1)
    assert (cols != np.arange(n)[:, None]).all() and (np.diff(cols, axis=1) > 0).all()
    g_indptr = torch.arange(n + 1, dtype=torch.int64, device="cuda") * k
    g_indices = torch.from_numpy(cols.astype(np.int32).ravel()).cuda()
    g_indptr, g_indices = _engine.neighbor_pool_graph("time_pool_neighbors", g_indptr, g_indices)
    # the same neighbourhoods as group lists: sorted N(i) per cell
    hoods = np.sort(np.concatenate([np.arange(n)[:, None], cols], axis=1), axis=1)
    rows = torch.from_numpy(hoods.astype(np.int64).ravel()).cuda()
    group_ptr = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (k + 1)
    shift = profile_shift(k + 1)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms)

    out = {"cells": n, "windows": w, "stored": nnz, "stored_fraction": nnz / (n * w), "neighbors": k, "shift": shift,
           "device": torch.cuda.get_device_name(0), "output_bytes": n * w * 8, "runs": []}
    pooled = torch.empty((n, w), dtype=torch.float64, device="cuda")
    other = torch.empty_like(pooled)
    out["copy_ms_median"], out["copy_ms_min"] = timed(lambda: other.copy_(pooled))
    out["copy_tb_per_s"] = 2 * n * w * 8 / (out["copy_ms_median"] * 1e-3) / 1e12
    del other
    n_cells, flags = _engine.neighbor_pool_sizes(g_indptr, g_indices)
    out["sizes_ms_median"], out["sizes_ms_min"] = timed(lambda: _engine.neighbor_pool_sizes(g_indptr, g_indices))
    assert int(n_cells.min().item()) == int(n_cells.max().item()) == k + 1 and int(flags.item()) == 0

    forms = {"csr_float64": (_engine.matrix_input(packed, "time_pool_neighbors"), (k + 1) * (12 * nnz + 16 * n)),
             "dense_float32": (_engine.matrix_input(dense32, "time_pool_neighbors"), (k + 1) * 4 * n * w)}
    bounds = chromosome_bounds({"chr1": 0}, w)
    for name, (dm, gathered) in forms.items():
        run = {"form": name, "gathered_bytes": gathered, "written_bytes": n * w * 8}
        run["pool_ms_median"], run["pool_ms_min"] = timed(
            lambda: _engine.neighbor_pool(dm, g_indptr, g_indices, shift, n_cells, flags, out=pooled))
        assert int(flags.item()) == 0

        def old_route():
            total, stored, _flags, d_ptr = _engine.group_profiles(dm, rows, group_ptr, shift)
            return _engine.group_profiles_finish(total, stored, d_ptr, shift)[0]

        run["group_profiles_route_ms_median"], run["group_profiles_route_ms_min"] = timed(old_route)
        run["same_bytes_as_the_group_profiles_route"] = bool(torch.equal(old_route().view(torch.int64), pooled.view(torch.int64)))
        run["pool_over_group_profiles_route"] = run["pool_ms_median"] / run["group_profiles_route_ms_median"]
        run["pool_written_plus_gathered_tb_per_s"] = (gathered + n * w * 8) / (run["pool_ms_median"] * 1e-3) / 1e12
        run["copy_time_over_pool_time"] = out["copy_ms_median"] / run["pool_ms_median"]
        torch.cuda.empty_cache()
        pdm = _engine.matrix_input(pooled, "time_pool_neighbors")
        sigma = math.sqrt(float((pooled * pooled).mean().item()))
        run["viterbi_ms_median"], run["viterbi_ms_min"] = timed(
            lambda: _engine.states_viterbi(pdm, bounds, amplitude=2.0 * sigma, h=1.0 / (2.0 * sigma * sigma),
                                           stay=math.log(1.0 - 1e-3), sw=math.log(1e-3 / 2.0)))
        out["runs"].append(run)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

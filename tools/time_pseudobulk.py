"""Times of tl.cnv_pseudobulk at the geometry of the tl.cnv_states figures (100 000 cells x 1 802 windows, 13 % stored,
float64 CSR, HBM-resident as tl.infercnv leaves it), for 6 groups and for 500.

    python tools/time_pseudobulk.py [--cells 100000] [--windows 1802] [--density 0.13] [--groups 6 500] [--reps 20]

Device-event times (median and minimum over --reps launches after a warm-up) of icv_group_profiles (its two memsets, the
slab table and the kernel) and of icv_group_profiles_finish, the bytes the first has to read (12 per stored entry, 16 per
row) over its time, next to the copy rate of HBM measured in the same run, and the host-clock time of the public call on
device input.  The same for the dense float32 form of the matrix.  The result is compared with a float64 numpy mean of
the same matrix: the largest difference has to stay within 2^-(shift + 1) and the float rounding of that sum."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--groups", type=int, nargs="+", default=[6, 500])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import pandas as pd
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine
    from infercnvpy_amd._compat import SimpleAnnData
    from infercnvpy_amd.tl._pseudobulk import profile_shift

    n, w = a.cells, a.windows
    gen = torch.Generator(device="cuda").manual_seed(0)
    keep = torch.rand((n, w), device="cuda", generator=gen) < a.density
    dense = torch.randn((n, w), device="cuda", generator=gen, dtype=torch.float64) * 0.5 * keep
    indptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    indptr[1:] = keep.sum(dim=1).cumsum(0)
    indices = keep.nonzero()[:, 1].to(torch.int32).contiguous()  # (row-major order: ascending columns in every row)
    packed = cnv.PackedCsr(indptr, indices, dense[keep].contiguous(), w)
    nnz = int(indptr[-1].item())
    dense32 = dense.to(torch.float32)
    del keep

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

    def clocked(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t), min(t)

    # the copy rate of HBM in this run: 1 GiB read and 1 GiB written
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy_ms, _ = timed(lambda: dst.copy_(src))
    hbm_tbs = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e12
    del src, dst

    out = {"cells": n, "windows": w, "stored": nnz, "stored_fraction": nnz / (n * w), "hbm_copy_tb_per_s": hbm_tbs,
           "device": torch.cuda.get_device_name(0), "runs": []}
    rng = np.random.default_rng(1)
    forms = {"csr_float64": (_engine.matrix_input(packed, "time_pseudobulk"), 12 * nnz + 16 * n, packed),
             "dense_float32": (_engine.matrix_input(dense32, "time_pseudobulk"), 4 * n * w + 8 * n, dense32)}
    for G in a.groups:
        codes = rng.integers(0, G, size=n)
        rows = torch.from_numpy(np.argsort(codes, kind="stable").astype(np.int64)).cuda()
        n_cells = np.bincount(codes, minlength=G)
        group_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64)).cuda()
        shift = profile_shift(int(n_cells.max()))
        for name, (dm, nbytes, x) in forms.items():
            run = {"form": name, "groups": G, "largest_group": int(n_cells.max()), "shift": shift, "bytes": nbytes}
            total, stored, flags, d_ptr = _engine.group_profiles(dm, rows, group_ptr, shift)
            run["profiles_ms_median"], run["profiles_ms_min"] = timed(lambda: _engine.group_profiles(dm, rows, group_ptr, shift))
            run["finish_ms_median"], run["finish_ms_min"] = timed(
                lambda: _engine.group_profiles_finish(total, stored, d_ptr, shift))
            run["profiles_tb_per_s"] = nbytes / (run["profiles_ms_median"] * 1e-3) / 1e12
            run["profiles_fraction_of_hbm_copy_rate"] = run["profiles_tb_per_s"] / hbm_tbs
            ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obs=pd.DataFrame({"clone": pd.Categorical(codes)}))
            ad.obsm["X_cnv"] = x
            ad.uns["cnv"] = {"chr_pos": {"chr1": 0}}
            run["call_ms_median"], run["call_ms_min"] = clocked(lambda: cnv.tl.cnv_pseudobulk(ad, "clone"))
            mean = cnv.tl.cnv_pseudobulk(ad, "clone").X
            ref = torch.zeros((G, w), dtype=torch.float64, device="cuda")
            ref.index_add_(0, torch.from_numpy(codes).cuda(), dense if name == "csr_float64" else dense32.to(torch.float64))
            ref /= torch.from_numpy(n_cells).cuda().to(torch.float64)[:, None]
            run["max_abs_difference_to_a_float64_mean"] = float((mean - ref).abs().max().item())
            run["resolution"] = 2.0 ** -(shift + 1)
            out["runs"].append(run)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Kernel times of tl.cnv_copy_posteriors and tl.cnv_copy_states_filter on an X_cnv-like matrix at the geometry of the
tl.cnv_posteriors figures (100 000 cells x 1 802 windows in 23 chromosomes, 13 % stored entries, HBM-resident as
tl.infercnv leaves it).

    python tools/time_copy_posteriors.py [--form csr|dense32] [--cells 100000] [--windows 1802] [--density 0.13] [--reps 20]

Device-event times, in one run, of icv_copy_posterior_chains with K = 3 (the levels (-a, 0, a)) and with K = 6 (the
default levels of tl.cnv_copy_states), the neutral plane alone and all K planes; of icv_posterior_chains, the specialised
three-state kernel, as the yardstick of the general one; and of icv_copy_states_filter next to icv_states_filter on the
three-state calls and posteriors of the same matrix: median and minimum over --reps launches after a warm-up, the LDS a
cell takes and the cells that fit a CU's 160 KiB beside each other.  --form csr reads the float64 CSR matrix, --form
dense32 the same values as a dense float32 matrix.  No time is a pass condition."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEFAULT_STEPS = (-2, -1, 0, 1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=("csr", "dense32"), default="csr")
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import torch

    from infercnvpy_amd import _engine, _lib
    from time_pca import synthetic_packed
    from time_states import chromosome_bounds

    x = synthetic_packed(a.cells, a.windows, a.density)
    nnz = x.nnz()
    cells_windows = a.cells * a.windows
    if a.form == "dense32":
        rows = torch.repeat_interleave(torch.arange(a.cells, device="cuda"), x.indptr[1:] - x.indptr[:-1])
        dense = torch.zeros((a.cells, a.windows), dtype=torch.float32, device="cuda")
        dense[rows, x.indices[:nnz].long()] = x.data[:nnz].float()
        del rows
        x, read = dense, 4 * cells_windows
    else:
        read = 12 * nnz + 8 * (a.cells + 1)
    dm = _engine.matrix_input(x, "time_copy_posteriors")
    bounds = chromosome_bounds(a.windows)
    n_chr = int(bounds.shape[0]) - 1
    q, flag = _engine.states_rowsq(dm)
    assert int(flag.item()) == 0
    sigma = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(a.cells) * float(a.windows)))
    amp, h, p = 2.0 * sigma, 1.0 / (2.0 * sigma * sigma), 1e-3
    models = {3: ((C.c_double * 3)(-amp, 0.0, amp), 1), 6: ((C.c_double * 6)(*(k * amp for k in DEFAULT_STEPS)), 2)}

    lib = _lib.load()
    m = dm.c_struct()
    ptr = _engine._ptr
    cs = torch.from_numpy(bounds).cuda()
    shape = (a.cells, a.windows)
    states = torch.empty(shape, dtype=torch.int8, device="cuda")
    count = torch.empty(a.cells, dtype=torch.int32, device="cuda")
    neutral, loss, gain = (torch.empty(shape, dtype=torch.float64, device="cuda") for _ in range(3))
    planes = torch.empty((6,) + shape, dtype=torch.float64, device="cuda")
    filtered, sign = (torch.empty(shape, dtype=torch.int8, device="cuda") for _ in range(2))
    kept = torch.empty(a.cells, dtype=torch.int32, device="cuda")
    removed = torch.empty(a.cells, dtype=torch.int32, device="cuda")
    bad = torch.empty(1, dtype=torch.int32, device="cuda")
    st = _engine._stream_ptr(torch)

    def general(k, all_planes):
        mu, z = models[k]
        return lambda: _lib.check(lib.icv_copy_posterior_chains(
            C.byref(m), ptr(cs), n_chr, mu, k, z, h, 1.0 - p, p / (k - 1), ptr(neutral),
            ptr(planes) if all_planes else None, st))

    def three_state(all_planes):
        return lambda: _lib.check(lib.icv_posterior_chains(
            C.byref(m), ptr(cs), n_chr, amp, h, 1.0 - p, p / 2.0, ptr(neutral), ptr(loss) if all_planes else None,
            ptr(gain) if all_planes else None, st))

    def copy_filter():
        _lib.check(lib.icv_copy_states_filter(ptr(states), ptr(neutral), a.cells, a.windows, ptr(cs), n_chr, 0.5,
                                              ptr(filtered), ptr(sign), ptr(kept), ptr(removed), ptr(bad), st))

    def filter_():
        _lib.check(lib.icv_states_filter(ptr(states), ptr(neutral), a.cells, a.windows, ptr(cs), n_chr, 0.5,
                                         ptr(filtered), ptr(kept), ptr(removed), ptr(bad), st))

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
        return {"ms_median": statistics.median(ms), "ms_min": min(ms)}

    out = {"form": a.form, "cells": a.cells, "windows": a.windows, "chromosomes": n_chr, "nnz": nnz,
           "density": nnz / cells_windows, "sigma": sigma, "reps": a.reps}
    for k in (3, 6):
        lds = 8 * (k + 1) * a.windows
        out[f"k{k}_lds_bytes_per_cell"] = lds
        out[f"k{k}_cells_per_cu_by_lds"] = _lib.ICV_COPY_POSTERIOR_LDS_BYTES // lds
        out[f"k{k}_neutral"] = dict(timed(general(k, False)), bytes=read + 8 * cells_windows)
        out[f"k{k}_all"] = dict(timed(general(k, True)), bytes=read + 8 * (k + 1) * cells_windows)
    out["three_state_lds_bytes_per_cell"] = 32 * a.windows
    out["three_state_cells_per_cu_by_lds"] = _lib.ICV_COPY_POSTERIOR_LDS_BYTES // (32 * a.windows)
    out["three_state_all"] = dict(timed(three_state(True)), bytes=read + 24 * cells_windows)
    out["three_state_neutral"] = dict(timed(three_state(False)), bytes=read + 8 * cells_windows)  # leaves P(neutral)
    _lib.check(lib.icv_states_viterbi(C.byref(m), ptr(cs), n_chr, amp, h, math.log(1.0 - p), math.log(p / 2.0),
                                      ptr(states), ptr(count), st))
    out["copy_states_filter"] = dict(timed(copy_filter), bytes=11 * cells_windows + 8 * a.cells)
    out["states_filter"] = dict(timed(filter_), bytes=10 * cells_windows + 8 * a.cells)
    assert int(bad.item()) == 0
    out["segments_removed"] = int(removed.sum().item())
    for name, num, den in (("general_k3_over_three_state_neutral", "k3_neutral", "three_state_neutral"),
                           ("general_k3_over_three_state_all", "k3_all", "three_state_all"),
                           ("k6_over_k3_neutral", "k6_neutral", "k3_neutral"), ("k6_over_k3_all", "k6_all", "k3_all"),
                           ("copy_filter_over_filter", "copy_states_filter", "states_filter")):
        out[name] = out[num]["ms_median"] / out[den]["ms_median"]
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

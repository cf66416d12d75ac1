"""Kernel times of tl.cnv_states on an X_cnv-like matrix at the geometry of the tl.pca figures (100 000 cells x 1 802
windows in 23 chromosomes, 13 % stored entries, float64 values, HBM-resident as tl.infercnv leaves it).

    python tools/time_states.py [--cells 100000] [--windows 1802] [--density 0.13] [--reps 20]

Device-event times of icv_states_rowsq and icv_states_viterbi (median and minimum over --reps launches after a warm-up),
the bytes the contract moves (12 per stored entry + 8 per row offset read, 1 per cell and window + 4 per cell written)
and the share of the measured HBM copy rate (6.29 TB/s) those bytes over the time amount to."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29  # measured float4 copy rate of one MI355X
# windows per chromosome in proportion to the human autosomes + X (Mbp)
CHROM_MBP = (248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51, 156)


def chromosome_bounds(w):
    total = float(sum(CHROM_MBP))
    cuts = np.round(np.cumsum((0,) + CHROM_MBP) / total * w).astype(np.int64)
    cuts = np.unique(np.clip(cuts, 0, w))
    return cuts.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import torch

    from infercnvpy_amd import _engine, _lib
    from time_pca import synthetic_packed

    x = synthetic_packed(a.cells, a.windows, a.density)
    nnz = x.nnz()
    dm = _engine.matrix_input(x, "time_states")
    bounds = chromosome_bounds(a.windows)
    q, flag = _engine.states_rowsq(dm)
    assert int(flag.item()) == 0
    sigma = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(a.cells) * float(a.windows)))
    amp, h = 2.0 * sigma, 1.0 / (2.0 * sigma * sigma)
    stay, sw = math.log(1.0 - 1e-3), math.log(1e-3 / 2.0)

    lib = _lib.load()
    m = dm.c_struct()
    cs = torch.from_numpy(bounds).cuda()
    states = torch.empty((a.cells, a.windows), dtype=torch.int8, device="cuda")
    count = torch.empty(a.cells, dtype=torch.int32, device="cuda")
    st = _engine._stream_ptr(torch)

    def rowsq():
        _lib.check(lib.icv_states_rowsq(C.byref(m), _engine._ptr(q), _engine._ptr(flag), st))

    def viterbi():
        _lib.check(lib.icv_states_viterbi(C.byref(m), _engine._ptr(cs), int(bounds.shape[0]) - 1, amp, h, stay, sw,
                                          _engine._ptr(states), _engine._ptr(count), st))

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

    v_med, v_min = timed(viterbi)
    r_med, r_min = timed(rowsq)
    v_bytes = 12 * nnz + 8 * (a.cells + 1) + a.cells * a.windows + 4 * a.cells
    r_bytes = 8 * nnz + 8 * (a.cells + 1) + 8 * a.cells
    print(json.dumps({
        "cells": a.cells, "windows": a.windows, "chromosomes": int(bounds.shape[0]) - 1, "nnz": nnz,
        "density": nnz / (a.cells * a.windows), "sigma": sigma,
        "nonneutral_fraction": float(count.sum().item()) / (a.cells * a.windows),
        "viterbi_ms_median": v_med, "viterbi_ms_min": v_min, "viterbi_bytes": v_bytes,
        "viterbi_tb_per_s": v_bytes / (v_med * 1e-3) / 1e12,
        "viterbi_fraction_of_hbm_rate": v_bytes / (v_med * 1e-3) / 1e12 / HBM_TBS,
        "rowsq_ms_median": r_med, "rowsq_ms_min": r_min, "rowsq_bytes": r_bytes,
        "rowsq_fraction_of_hbm_rate": r_bytes / (r_med * 1e-3) / 1e12 / HBM_TBS,
        "device": torch.cuda.get_device_name(0),
    }), flush=True)


if __name__ == "__main__":
    main()

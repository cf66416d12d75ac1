"""Kernel times of tl.cnv_posteriors and tl.cnv_states_filter on an X_cnv-like matrix at the geometry of the tl.pca and
tl.cnv_states figures (100 000 cells x 1 802 windows in 23 chromosomes, 13 % stored entries, float64 values,
HBM-resident as tl.infercnv leaves it).

    python tools/time_posteriors.py [--cells 100000] [--windows 1802] [--density 0.13] [--reps 20]

Device-event times of icv_posterior_chains (the neutral plane alone and all three planes), of icv_states_filter on the
calls and posteriors of the same matrix, and of icv_states_viterbi as the yardstick (the same geometry, half the
passes): median and minimum over --reps launches after a warm-up, with the bytes each contract moves."""
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
    from time_states import chromosome_bounds

    x = synthetic_packed(a.cells, a.windows, a.density)
    nnz = x.nnz()
    dm = _engine.matrix_input(x, "time_posteriors")
    bounds = chromosome_bounds(a.windows)
    n_chr = int(bounds.shape[0]) - 1
    q, flag = _engine.states_rowsq(dm)
    assert int(flag.item()) == 0
    sigma = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(a.cells) * float(a.windows)))
    amp, h, p = 2.0 * sigma, 1.0 / (2.0 * sigma * sigma), 1e-3
    stay, sw, ps, pw = math.log(1.0 - p), math.log(p / 2.0), 1.0 - p, p / 2.0

    lib = _lib.load()
    m = dm.c_struct()
    ptr = _engine._ptr
    cs = torch.from_numpy(bounds).cuda()
    shape = (a.cells, a.windows)
    states = torch.empty(shape, dtype=torch.int8, device="cuda")
    count = torch.empty(a.cells, dtype=torch.int32, device="cuda")
    neutral, loss, gain = (torch.empty(shape, dtype=torch.float64, device="cuda") for _ in range(3))
    filtered = torch.empty(shape, dtype=torch.int8, device="cuda")
    kept = torch.empty(a.cells, dtype=torch.int32, device="cuda")
    removed = torch.empty(a.cells, dtype=torch.int32, device="cuda")
    bad = torch.empty(1, dtype=torch.int32, device="cuda")
    st = _engine._stream_ptr(torch)

    def viterbi():
        _lib.check(lib.icv_states_viterbi(C.byref(m), ptr(cs), n_chr, amp, h, stay, sw, ptr(states), ptr(count), st))

    def chains_neutral():
        _lib.check(lib.icv_posterior_chains(C.byref(m), ptr(cs), n_chr, amp, h, ps, pw, ptr(neutral), None, None, st))

    def chains_all():
        _lib.check(lib.icv_posterior_chains(C.byref(m), ptr(cs), n_chr, amp, h, ps, pw, ptr(neutral), ptr(loss),
                                            ptr(gain), st))

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
        return statistics.median(ms), min(ms)

    v_med, v_min = timed(viterbi)
    n_med, n_min = timed(chains_neutral)
    a_med, a_min = timed(chains_all)
    f_med, f_min = timed(filter_)
    assert int(bad.item()) == 0
    cells_windows = a.cells * a.windows
    read = 12 * nnz + 8 * (a.cells + 1)
    print(json.dumps({
        "cells": a.cells, "windows": a.windows, "chromosomes": n_chr, "nnz": nnz, "density": nnz / cells_windows,
        "sigma": sigma, "nonneutral_fraction": float(count.sum().item()) / cells_windows,
        "segments_removed": int(removed.sum().item()),
        "viterbi_ms_median": v_med, "viterbi_ms_min": v_min, "viterbi_bytes": read + cells_windows + 4 * a.cells,
        "posterior_neutral_ms_median": n_med, "posterior_neutral_ms_min": n_min,
        "posterior_neutral_bytes": read + 8 * cells_windows,
        "posterior_all_ms_median": a_med, "posterior_all_ms_min": a_min, "posterior_all_bytes": read + 24 * cells_windows,
        "posterior_neutral_over_viterbi": n_med / v_med,
        "filter_ms_median": f_med, "filter_ms_min": f_min, "filter_bytes": 10 * cells_windows + 8 * a.cells,
        "device": torch.cuda.get_device_name(0),
    }), flush=True)


if __name__ == "__main__":
    main()

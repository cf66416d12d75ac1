"""Kernel time of the E-step of tl.cnv_copy_states_fit on an X_cnv-like matrix at the geometry of the tl.cnv_states_fit
figures (100 000 cells x 1 802 windows in 23 chromosomes, 13 % stored entries, float64 CSR, HBM-resident as tl.infercnv
leaves it).

    python tools/time_copy_fit.py [--cells 100000] [--windows 1802] [--density 0.13] [--reps 20] [--states 3 6]

For every K of --states: device-event times of icv_copy_posterior_stats and, as the yardstick in the same run, of
icv_copy_posterior_chains (the neutral plane alone: the same recursions without the 2K + 1 sums, and 8 W bytes stored per
cell instead of 8 (2K + 1)): median and minimum over --reps launches after a warm-up.  K = 3 runs the levels (-a, 0, a),
K = 6 the default lattice (-2 .. 3) a, a = 2 sigma and sigma the root mean square.  Then the host clock of one default
tl.cnv_copy_states_fit call on the same matrix (start values, every E-step with its read-back of n x 13 sums, the
M-steps), with its iterations."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LATTICE = {2: (0, 1), 3: (-1, 0, 1), 4: (-1, 0, 1, 2), 5: (-2, -1, 0, 1, 2), 6: (-2, -1, 0, 1, 2, 3),
           7: (-3, -2, -1, 0, 1, 2, 3), 8: (-3, -2, -1, 0, 1, 2, 3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--states", type=int, nargs="+", default=[3, 6], choices=sorted(LATTICE))
    a = ap.parse_args()

    import numpy as np
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib
    from infercnvpy_amd._compat import SimpleAnnData
    from time_pca import synthetic_packed
    from time_states import chromosome_bounds

    x = synthetic_packed(a.cells, a.windows, a.density)
    nnz = x.nnz()
    dm = _engine.matrix_input(x, "time_copy_fit")
    bounds = chromosome_bounds(a.windows)
    n_chr = int(bounds.shape[0]) - 1
    q, flag = _engine.states_rowsq(dm)
    assert int(flag.item()) == 0
    sigma = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(a.cells) * float(a.windows)))
    amp, h, p = 2.0 * sigma, 1.0 / (2.0 * sigma * sigma), 1e-3

    lib = _lib.load()
    m = dm.c_struct()
    ptr = _engine._ptr
    cs = torch.from_numpy(bounds).cuda()
    neutral = torch.empty((a.cells, a.windows), dtype=torch.float64, device="cuda")
    st = _engine._stream_ptr(torch)

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

    cells_windows = a.cells * a.windows
    read = 12 * nnz + 8 * (a.cells + 1)
    per_k = {}
    for k in a.states:
        lattice = LATTICE[k]
        z = lattice.index(0)
        mu = (C.c_double * k)(*(float(s) * amp for s in lattice))
        ps, pw = 1.0 - p, p / (k - 1)
        stats = torch.empty((a.cells, 2 * k + 1), dtype=torch.float64, device="cuda")

        def chains_neutral():
            _lib.check(lib.icv_copy_posterior_chains(C.byref(m), ptr(cs), n_chr, mu, k, z, h, ps, pw, ptr(neutral), None, st))

        def e_step():
            _lib.check(lib.icv_copy_posterior_stats(C.byref(m), ptr(cs), n_chr, mu, k, z, h, ps, pw, ptr(stats), st))

        c_med, c_min = timed(chains_neutral)
        s_med, s_min = timed(e_step)
        sums = stats.sum(0).cpu().tolist()
        per_k[str(k)] = {
            "steps": list(lattice), "lds_bytes": _lib.ICV_COPY_POSTERIOR_STATS_LDS(a.windows, k, n_chr),
            "neutral_mass": sums[z] / cells_windows,
            "copy_posterior_neutral_ms_median": c_med, "copy_posterior_neutral_ms_min": c_min,
            "copy_posterior_neutral_bytes": read + 8 * cells_windows,
            "copy_posterior_stats_ms_median": s_med, "copy_posterior_stats_ms_min": s_min,
            "copy_posterior_stats_bytes": read + 8 * (2 * k + 1) * a.cells,
            "stats_over_neutral": s_med / c_med,
        }
    del neutral

    ad = SimpleAnnData(np.zeros((a.cells, 1), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": {f"chr{c + 1}": int(s) for c, s in enumerate(bounds[:-1])}}
    cnv.tl.cnv_copy_states_fit(ad, max_iter=1)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, info = cnv.tl.cnv_copy_states_fit(ad, return_info=True)
    fit_ms = (time.perf_counter() - t0) * 1e3

    print(json.dumps({
        "cells": a.cells, "windows": a.windows, "chromosomes": n_chr, "nnz": nnz, "density": nnz / cells_windows,
        "sigma": sigma, "states": per_k,
        "fit_ms": fit_ms, "fit_iterations": info["n_iter"], "fit_converged": info["converged"],
        "fit_ms_per_iteration": info["stage_ms"]["e_steps"] / max(info["n_iter"], 1), "fit_stage_ms": info["stage_ms"],
        "fit_start": info["history"][0], "fit_amplitude": info["amplitude"],
        "fit_params": ad.uns["cnv_copy_states_fit"]["params"],
        "device": torch.cuda.get_device_name(0),
    }), flush=True)


if __name__ == "__main__":
    main()

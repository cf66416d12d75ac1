"""Kernel times of tl.cnv_copy_states on an X_cnv-like matrix at the geometry of the tl.cnv_states figures (100 000 cells x
1 802 windows in 23 chromosomes, 13 % stored entries, HBM-resident).

    python tools/time_copy_states.py [--cells 100000] [--windows 1802] [--density 0.13] [--reps 20]

Device-event times (median and minimum over --reps launches after a warm-up) of icv_copy_states_viterbi with K = 3
(the levels (-a, 0, a): the model of icv_states_viterbi) and K = 6 (the default levels k a, k = -2 .. 3), and of
icv_states_viterbi in the same run as the yardstick; the K = 3 bytes are checked against the yardstick's.  Two forms of
the matrix: float64 CSR as tl.infercnv leaves it, and the same matrix as dense float32.  Each form is measured in a
process of its own, started under its own ``timeout``; the first that fails ends the run.  One JSON line per form."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FORMS = ("csr_float64", "dense_float32")
STEP_SECONDS = 240  # the time limit of one form


def measure(a):
    import torch

    from infercnvpy_amd import _engine, _lib
    from time_pca import synthetic_packed
    from time_states import chromosome_bounds

    x = synthetic_packed(a.cells, a.windows, a.density)
    nnz = x.nnz()
    if a.form == "dense_float32":
        rows = torch.repeat_interleave(torch.arange(a.cells, device="cuda"), x.indptr[1:] - x.indptr[:-1])
        dense = torch.zeros((a.cells, a.windows), dtype=torch.float32, device="cuda")
        dense[rows, x.indices[:nnz].long()] = x.data[:nnz].float()
        del rows
        x = dense
    dm = _engine.matrix_input(x, "time_copy_states")
    bounds = chromosome_bounds(a.windows)
    n_chr = int(bounds.shape[0]) - 1
    q, flag = _engine.states_rowsq(dm)
    assert int(flag.item()) == 0
    sigma = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(a.cells) * float(a.windows)))
    amp, h, p = 2.0 * sigma, 1.0 / (2.0 * sigma * sigma), 1e-3
    stay = math.log(1.0 - p)

    lib = _lib.load()
    m = dm.c_struct()
    ptr = _engine._ptr
    cs = torch.from_numpy(bounds).cuda()
    shape = (a.cells, a.windows)
    three, states, sign = (torch.empty(shape, dtype=torch.int8, device="cuda") for _ in range(3))
    count3, count = (torch.empty(a.cells, dtype=torch.int32, device="cuda") for _ in range(2))
    st = _engine._stream_ptr(torch)
    mu3 = (C.c_double * 3)(-amp, 0.0, amp)
    mu6 = (C.c_double * 6)(*(float(k) * amp for k in (-2, -1, 0, 1, 2, 3)))

    def yardstick():
        _lib.check(lib.icv_states_viterbi(C.byref(m), ptr(cs), n_chr, amp, h, stay, math.log(p / 2.0), ptr(three),
                                          ptr(count3), st))

    def copy_states(mu, neutral):
        def fn():
            _lib.check(lib.icv_copy_states_viterbi(C.byref(m), ptr(cs), n_chr, mu, len(mu), neutral, h, stay,
                                                   math.log(p / (len(mu) - 1)), ptr(states), ptr(sign), ptr(count), st))
        return fn

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

    y_med, y_min = timed(yardstick)
    k3_med, k3_min = timed(copy_states(mu3, 1))
    same = bool(torch.equal(states, three)) and bool(torch.equal(sign, three)) and bool(torch.equal(count, count3))
    k6_med, k6_min = timed(copy_states(mu6, 2))
    cells_windows = a.cells * a.windows
    read = 12 * nnz + 8 * (a.cells + 1) if a.form == "csr_float64" else 4 * cells_windows
    print(json.dumps({
        "form": a.form, "cells": a.cells, "windows": a.windows, "chromosomes": n_chr, "nnz": nnz, "sigma": sigma,
        "states_viterbi_ms_median": y_med, "states_viterbi_ms_min": y_min,
        "states_viterbi_bytes": read + cells_windows + 4 * a.cells,
        "copy_states_k3_ms_median": k3_med, "copy_states_k3_ms_min": k3_min,
        "copy_states_k6_ms_median": k6_med, "copy_states_k6_ms_min": k6_min,
        "copy_states_bytes": read + 2 * cells_windows + 4 * a.cells,
        "k3_over_states_viterbi": k3_med / y_med, "k6_over_k3": k6_med / k3_med,
        "k3_equals_states_viterbi": same,
        "k6_nonneutral_fraction": float(count.sum().item()) / cells_windows,
        "k6_beyond_one_step_fraction": float((states != sign).sum().item()) / cells_windows,
        "device": torch.cuda.get_device_name(0),
    }), flush=True)
    assert same, "K = 3 does not give the bytes of icv_states_viterbi"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--form", choices=FORMS, help="measure this form in this process (what the run starts per form)")
    a = ap.parse_args()
    if a.form:
        measure(a)
        return 0
    for form in FORMS:
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--cells",
                             str(a.cells), "--windows", str(a.windows), "--density", str(a.density), "--reps", str(a.reps),
                             "--form", form]).returncode
        if rc != 0:
            print(f"time_copy_states: the {form} step ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

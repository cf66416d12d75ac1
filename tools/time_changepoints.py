"""Times of tl.cnv_changepoints' two kernels at the geometry of the tl.cnv_states figures (100 000 cells x 1 802 windows in
23 chromosomes, 13 % stored, float64 CSR, HBM-resident as tl.infercnv leaves it) and on 6 dense rows (clone profiles).

    python tools/time_changepoints.py [--cells 100000] [--windows 1802] [--density 0.13] [--reps 20]
                                      [--layout-cells 20000] [--layouts 16 32 64 128 256 901]

Device-event times (median and minimum over --reps launches after a warm-up) of icv_changepoint_levels and
icv_changepoint_diffsq, and in the same run of the two yardsticks that walk the same rows chromosome by chromosome,
icv_states_viterbi and icv_posterior_chains.  To see what bounds icv_changepoint_levels the same windows are then cut into
chromosomes of one length each (--layouts, on --layout-cells rows): a launch takes one step per window (the reduction
over the lanes, the write of F_j and the barrier) and one batch of 64 candidates per 64 admissible i of every step (the
division of rule 2); the least-squares fit of ``time = a steps + b batches`` over the layouts gives the cost of each."""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layout-cells", type=int, default=20000)
    ap.add_argument("--layouts", type=int, nargs="*", default=[16, 32, 64, 128, 256, 901])
    a = ap.parse_args()

    import torch

    from infercnvpy_amd import _engine, _lib
    from infercnvpy_amd.tl._changepoints import default_sigma
    from time_pca import synthetic_packed
    from time_states import chromosome_bounds

    n, w = a.cells, a.windows
    packed = synthetic_packed(n, w, a.density)
    nnz = packed.nnz()
    dm = _engine.matrix_input(packed, "time_changepoints")
    lib = _lib.load()
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

    bounds = chromosome_bounds(w)
    n_chr = int(bounds.shape[0]) - 1
    lengths = np.diff(bounds)
    print(f"device: {torch.cuda.get_device_name(0)}; {n} cells x {w} windows in {n_chr} chromosomes of {lengths.min()} to "
          f"{lengths.max()} windows, {nnz} stored ({nnz / (n * w):.3f}), median / minimum of {a.reps} launches, device events",
          flush=True)

    # ---- the yardsticks ----------------------------------------------------------------------------------------------------
    q, _ = _engine.states_rowsq(dm)
    rms = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(n) * float(w)))
    h = 1.0 / (2.0 * rms * rms)
    cs = torch.from_numpy(bounds).cuda()
    m = dm.c_struct()
    states = torch.empty((n, w), dtype=torch.int8, device="cuda")
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    vt_ms, vt_min = timed(lambda: _lib.check(lib.icv_states_viterbi(
        C.byref(m), _engine._ptr(cs), n_chr, 2.0 * rms, h, math.log(1.0 - 1e-3), math.log(1e-3 / 2.0), _engine._ptr(states),
        _engine._ptr(count), st)))
    del states
    neutral = torch.empty((n, w), dtype=torch.float64, device="cuda")
    po_ms, po_min = timed(lambda: _lib.check(lib.icv_posterior_chains(
        C.byref(m), _engine._ptr(cs), n_chr, 2.0 * rms, h, 1.0 - 1e-3, 1e-3 / 2.0, _engine._ptr(neutral), None, None, st)))
    del neutral
    print(f"yardstick icv_states_viterbi:   {vt_ms:.3f} / {vt_min:.3f} ms")
    print(f"yardstick icv_posterior_chains: {po_ms:.3f} / {po_min:.3f} ms", flush=True)

    # ---- the two kernels -----------------------------------------------------------------------------------------------------
    def work(edges):
        """(steps, batches of 64 candidates) of one row."""
        steps = batches = 0
        for length in np.diff(edges).tolist():
            steps += length
            batches += sum((j + 63) // 64 for j in range(1, length + 1))
        return steps, batches

    def levels_ms(mat, edges, beta, shortest=1):
        rows, width = mat.shape
        d_cs = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32)).cuda()
        ms_ = mat.c_struct()
        levels = torch.empty((rows, width), dtype=torch.float64, device="cuda")
        starts = torch.empty((rows, width), dtype=torch.uint8, device="cuda")
        out = timed(lambda: _lib.check(lib.icv_changepoint_levels(
            C.byref(ms_), _engine._ptr(d_cs), int(len(edges)) - 1, beta, shortest, _engine._ptr(levels), _engine._ptr(starts), st)))
        return out, int(starts.sum().item())

    ds_ms, ds_min = timed(lambda: _engine.changepoint_diffsq(dm, bounds))
    sigma = default_sigma(_engine.changepoint_diffsq(dm, bounds).cpu().numpy().tolist(), n, w, n_chr)
    beta = (2.0 * (sigma * sigma)) * math.log(w)
    (lv_ms, lv_min), n_seg = levels_ms(dm, bounds, beta)
    steps, batches = work(bounds)
    print(f"icv_changepoint_diffsq: {ds_ms:.3f} / {ds_min:.3f} ms = {ds_ms / vt_ms:.2f} x viterbi; sigma = {sigma:.4f} "
          f"(rms {rms:.4f})")
    print(f"icv_changepoint_levels: {lv_ms:.3f} / {lv_min:.3f} ms = {lv_ms / vt_ms:.2f} x viterbi, {lv_ms / po_ms:.2f} x "
          f"posterior_chains; {n_seg / n:.2f} segments per row; {n * batches * 64 / (lv_ms * 1e-3) / 1e9:.1f} G candidates/s "
          f"({steps} steps and {batches} batches per row)", flush=True)
    (l5_ms, l5_min), _ = levels_ms(dm, bounds, beta, 5)
    print(f"icv_changepoint_levels, min_windows = 5: {l5_ms:.3f} / {l5_min:.3f} ms")

    six = packed.dense_rows(np.arange(6)).double().contiguous()
    dm6 = _engine.matrix_input(six, "time_changepoints")
    (c_ms, c_min), _ = levels_ms(dm6, bounds, beta)
    d6_ms, d6_min = timed(lambda: _engine.changepoint_diffsq(dm6, bounds))
    print(f"6 dense rows: icv_changepoint_levels {c_ms:.3f} / {c_min:.3f} ms, icv_changepoint_diffsq {d6_ms:.3f} / "
          f"{d6_min:.3f} ms", flush=True)

    # ---- what bounds it: chromosomes of one length ---------------------------------------------------------------------------
    if a.layouts:
        rows = min(n, a.layout_cells)
        sub = _engine.matrix_input(synthetic_packed(rows, w, a.density, seed=1), "time_changepoints")
        table = []
        for length in a.layouts:
            edges = np.unique(np.concatenate([np.arange(0, w, length), [w]])).astype(np.int32)
            (ms, lo), _ = levels_ms(sub, edges, beta)
            s, b = work(edges)
            table.append((s, b, ms))
            print(f"chromosomes of {length:4d} windows ({len(edges) - 1:3d} per row, {rows} rows): {ms:8.3f} / {lo:8.3f} ms; "
                  f"{s} steps, {b} batches per row", flush=True)
        if len(table) >= 2:
            A = np.asarray([[t[0], t[1]] for t in table], dtype=np.float64) * rows
            coef, *_ = np.linalg.lstsq(A, np.asarray([t[2] for t in table]) * 1e6, rcond=None)  # ns per unit over the device
            fit = A @ coef / 1e6
            print(f"fit: {coef[0]:.4f} ns per step and {coef[1]:.4f} ns per batch of 64 candidates over the whole device; "
                  f"fitted / measured = " + ", ".join(f"{f / t[2]:.2f}" for f, t in zip(fit, table)))
            print(f"at the 23-chromosome layout the steps take {coef[0] * steps * n / 1e6:.2f} ms and the batches "
                  f"{coef[1] * batches * n / 1e6:.2f} ms of the measured {lv_ms:.2f} ms")


if __name__ == "__main__":
    main()

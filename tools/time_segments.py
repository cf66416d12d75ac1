"""Times of tl.cnv_segments on a planted call matrix at the geometry of the tl.cnv_states figures (100 000 cells x 1 802
windows in 23 chromosomes, int8, HBM-resident as tl.cnv_states leaves it; 6 groups).

    python tools/time_segments.py [--cells 100000] [--windows 1802] [--groups 6] [--reps 20]

Device-event times (median and minimum over --reps launches after a warm-up) of the per-cell chain (icv_segments_count,
icv_row_offsets, icv_segments_fill) and of the per-group chain (icv_state_votes, icv_state_consensus and count / scan /
fill / support on the G x W consensus), each kernel stage on its own as well, the bytes each stage has to move over its
time as a share of the measured HBM copy rate (6.29 TB/s), and host-clock times of the two public calls (device input,
tables on the host).  Next to it a vectorised numpy baseline on the same box: np.diff on the padded matrix for the
segments, np.add.at for the votes."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29  # measured float4 copy rate of one MI355X
CHROM_MBP = (248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51, 156)


def chromosome_bounds(w):
    total = float(sum(CHROM_MBP))
    cuts = np.round(np.cumsum((0,) + CHROM_MBP) / total * w).astype(np.int64)
    return np.unique(np.clip(cuts, 0, w)).astype(np.int32)


def planted_states(n, bounds, n_groups, seed=0):
    """int8 n x W: every group has a gain or loss block of 20 .. 120 windows in half of the chromosomes, 90 % of its cells
    carry each block, and every cell has private blocks of 5 .. 15 windows in a quarter of the chromosomes."""
    rng = np.random.default_rng(seed)
    w = int(bounds[-1])
    codes = rng.integers(0, n_groups, size=n)
    S = np.zeros((n, w), dtype=np.int8)
    for a, b in zip(bounds[:-1], bounds[1:]):
        length = int(b - a)
        for g in range(n_groups):
            if rng.random() < 0.5 and length > 20:
                seg = int(rng.integers(20, min(length, 120) + 1))
                off = int(a) + int(rng.integers(0, length - seg + 1))
                cells = np.flatnonzero((codes == g) & (rng.random(n) < 0.9))
                S[cells, off:off + seg] = 1 if rng.random() < 0.5 else -1
        if length >= 15:
            own = np.flatnonzero(rng.random(n) < 0.25)
            seg = rng.integers(5, 16, size=own.shape[0])
            off = int(a) + np.floor(rng.random(own.shape[0]) * (length - seg + 1)).astype(np.int64)
            sign = np.where(rng.random(own.shape[0]) < 0.5, -1, 1).astype(np.int8)
            for i, o, k, s in zip(own.tolist(), off.tolist(), seg.tolist(), sign.tolist()):
                S[i, o:o + k] = s
    return S, codes


def numpy_segments(S, bounds):
    """(row, start, end, state) of every run: np.diff on the matrix padded with a neutral column, per chromosome."""
    rows, starts, ends, states = [], [], [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        blk = np.zeros((S.shape[0], int(b - a) + 2), dtype=np.int8)
        blk[:, 1:-1] = S[:, a:b]
        change = np.diff(blk, axis=1) != 0
        r0, c0 = np.nonzero(change[:, :-1] & (blk[:, 1:-1] != 0))
        r1, c1 = np.nonzero(change[:, 1:] & (blk[:, 1:-1] != 0))
        rows.append(r0), starts.append(c0 + a), ends.append(c1 + a + 1), states.append(blk[r0, c0 + 1])
    row, start = np.concatenate(rows), np.concatenate(starts)
    order = np.lexsort((start, row))
    return row[order], start[order], np.concatenate(ends)[order], np.concatenate(states)[order]


def numpy_votes(S, codes, n_groups):
    loss = np.zeros((n_groups, S.shape[1]), dtype=np.int32)
    gain = np.zeros((n_groups, S.shape[1]), dtype=np.int32)
    np.add.at(loss, codes, S == -1)
    np.add.at(gain, codes, S == 1)
    return loss, gain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--groups", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import pandas as pd
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib
    from infercnvpy_amd._compat import SimpleAnnData

    bounds = chromosome_bounds(a.windows)
    S, codes = planted_states(a.cells, bounds, a.groups)
    n, w, G = a.cells, a.windows, a.groups
    lib = _lib.load()
    ptr, st = _engine._ptr, _engine._stream_ptr(torch)
    d_S = torch.from_numpy(S).cuda()
    cs = torch.from_numpy(bounds).cuda()
    n_chr = int(bounds.shape[0]) - 1

    # ---- per cell: count, scan, fill --------------------------------------------------------------------------------------
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    bad = torch.empty(1, dtype=torch.int32, device="cuda")

    def count():
        _lib.check(lib.icv_segments_count(ptr(d_S), n, w, ptr(cs), n_chr, ptr(counts), ptr(bad), st))

    def scan():
        _lib.check(lib.icv_row_offsets(ptr(counts), n, ptr(offsets), st))

    count(), scan()
    n_seg = int(offsets[-1].item())
    assert int(bad.item()) == 0
    seg_row = torch.empty(n_seg, dtype=torch.int64, device="cuda")
    seg_start = torch.empty(n_seg, dtype=torch.int32, device="cuda")
    seg_end = torch.empty(n_seg, dtype=torch.int32, device="cuda")
    seg_state = torch.empty(n_seg, dtype=torch.int8, device="cuda")

    def fill():
        _lib.check(lib.icv_segments_fill(ptr(d_S), n, w, ptr(cs), n_chr, ptr(offsets), n_seg, ptr(seg_row), ptr(seg_start),
                                         ptr(seg_end), ptr(seg_state), st))

    # ---- per group: votes, consensus, count / scan / fill / support on G x W --------------------------------------------------
    rows = torch.from_numpy(np.argsort(codes, kind="stable").astype(np.int64)).cuda()
    n_cells = np.bincount(codes, minlength=G)
    group_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64)).cuda()
    need = torch.from_numpy(np.maximum(1, -(-n_cells // 2)).astype(np.int32)).cuda()
    loss = torch.empty((G, w), dtype=torch.int32, device="cuda")
    gain = torch.empty((G, w), dtype=torch.int32, device="cuda")
    consensus = torch.empty((G, w), dtype=torch.int8, device="cuda")

    def votes():
        _lib.check(lib.icv_state_votes(ptr(d_S), n, w, ptr(rows), n, ptr(group_ptr), G, ptr(loss), ptr(gain), ptr(bad), st))

    def cons():
        _lib.check(lib.icv_state_consensus(ptr(loss), ptr(gain), ptr(need), G, w, ptr(consensus), st))

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

    out = {"cells": n, "windows": w, "chromosomes": n_chr, "groups": G, "segments": n_seg,
           "nonneutral_fraction": float((S != 0).mean()), "device": torch.cuda.get_device_name(0)}
    matrix = n * w
    stages = {"count": (count, matrix + 8 * n), "scan": (scan, 16 * n), "fill": (fill, matrix + 8 * n + 17 * n_seg),
              "votes": (votes, matrix + 8 * n + 2 * 4 * G * w), "consensus": (cons, 9 * G * w)}
    for name, (fn, nbytes) in stages.items():
        med, lo = timed(fn)
        out[name + "_ms_median"], out[name + "_ms_min"], out[name + "_bytes"] = med, lo, nbytes
        out[name + "_fraction_of_hbm_rate"] = nbytes / (med * 1e-3) / 1e12 / HBM_TBS

    # the public calls on device input: everything they do, tables copied to the host and made a DataFrame
    ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obs=pd.DataFrame({"clone": pd.Categorical(codes)}))
    ad.obsm["X_cnv_states"] = d_S
    ad.uns["cnv"] = {"chr_pos": {f"chr{c + 1}": int(s) for c, s in enumerate(bounds[:-1])}}
    out["call_cells_ms_median"], out["call_cells_ms_min"] = clocked(lambda: cnv.tl.cnv_segments(ad, inplace=False))
    out["call_groups_ms_median"], out["call_groups_ms_min"] = clocked(lambda: cnv.tl.cnv_segments(ad, "clone", inplace=False))
    table, d_cons, d_loss, d_gain = cnv.tl.cnv_segments(ad, "clone", inplace=False)
    out["group_segments"] = int(len(table))

    # the numpy baseline on this box, and its agreement with the device
    t0 = time.perf_counter()
    h_row, h_start, h_end, h_state = numpy_segments(S, bounds)
    out["numpy_segments_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    h_loss, h_gain = numpy_votes(S, codes, G)
    out["numpy_votes_ms"] = (time.perf_counter() - t0) * 1e3
    fill()
    out["equal_to_numpy"] = bool(
        np.array_equal(seg_row.cpu().numpy(), h_row) and np.array_equal(seg_start.cpu().numpy(), h_start)
        and np.array_equal(seg_end.cpu().numpy(), h_end) and np.array_equal(seg_state.cpu().numpy(), h_state)
        and np.array_equal(d_loss, h_loss) and np.array_equal(d_gain, h_gain))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Times of tl.cnv_rank_groups at the geometry of the tl.cnv_states figures (100 000 cells x 1 802 windows in 23
chromosomes, 13 % stored, float64 CSR, HBM-resident as tl.infercnv leaves it), for 6 groups and for 500.

    python tools/time_rank_groups.py [--cells 100000] [--windows 1802] [--density 0.13] [--groups 6 500] [--reps 20]
                                     [--host-cells 20000]

Device-event times per stage of the ranking (count, scatter, sort, rank sums, finish: median and minimum over --reps runs
of _engine.rank_tables after a warm-up), the whole public call on the host clock, and in the same run the yardsticks that
read the same 12 bytes per stored entry, icv_group_profiles and icv_states_viterbi, and the copy rate of HBM.  The host
baseline is scipy.stats.rankdata(axis=0) plus the group sums (a one-hot sparse product) on the first --host-cells cells of
the same matrix, whose doubled rank sums are compared with the device's for those cells.  One JSON line at the end."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--groups", type=int, nargs="+", default=[6, 500])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-cells", type=int, default=20000)
    a = ap.parse_args()

    import pandas as pd
    import scipy.sparse
    import scipy.stats
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib
    from infercnvpy_amd._compat import SimpleAnnData
    from infercnvpy_amd.tl._pseudobulk import profile_shift
    from time_pca import synthetic_packed
    from time_states import chromosome_bounds

    n, w = a.cells, a.windows
    packed = synthetic_packed(n, w, a.density)
    nnz = packed.nnz()
    dm = _engine.matrix_input(packed, "time_rank_groups")
    lib = _lib.load()
    st = _engine._stream_ptr(torch)
    bounds = chromosome_bounds(w)
    chr_pos = {f"chr{i + 1}": int(s) for i, s in enumerate(bounds[:-1])}

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

    print(f"device: {torch.cuda.get_device_name(0)}; {n} cells x {w} windows in {len(chr_pos)} chromosomes, {nnz} stored "
          f"({nnz / (n * w):.3f}), median / minimum of {a.reps} runs, device events", flush=True)
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()  # 1 GiB read and 1 GiB written
    dst = torch.empty_like(src)
    copy_ms, _ = timed(lambda: dst.copy_(src))
    hbm = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e12
    del src, dst
    print(f"HBM copy rate of this run: {hbm:.2f} TB/s", flush=True)
    out = {"cells": n, "windows": w, "chromosomes": len(chr_pos), "stored": nnz, "hbm_copy_tb_per_s": hbm,
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "runs": []}

    # ---- the yardstick that does not depend on the groups --------------------------------------------------------------------
    q, _ = _engine.states_rowsq(dm)
    sigma = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(n) * float(w)))
    cs = torch.from_numpy(bounds).cuda()
    states = torch.empty((n, w), dtype=torch.int8, device="cuda")
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    m = dm.c_struct()

    def viterbi():
        _lib.check(lib.icv_states_viterbi(C.byref(m), _engine._ptr(cs), int(bounds.shape[0]) - 1, 2.0 * sigma,
                                          1.0 / (2.0 * sigma * sigma), math.log(1.0 - 1e-3), math.log(1e-3 / 2.0),
                                          _engine._ptr(states), _engine._ptr(count), st))

    out["viterbi_ms_median"], out["viterbi_ms_min"] = timed(viterbi)
    del states
    print(f"yardstick icv_states_viterbi: {out['viterbi_ms_median']:.3f} / {out['viterbi_ms_min']:.3f} ms", flush=True)

    rng = np.random.default_rng(1)
    for G in a.groups:
        codes = rng.integers(0, G, size=n)
        n_cells = np.bincount(codes, minlength=G).astype(np.int64)
        run = {"groups": G, "largest_group": int(n_cells.max())}
        rows = torch.from_numpy(np.argsort(codes, kind="stable").astype(np.int64)).cuda()
        group_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64)).cuda()
        shift = profile_shift(int(n_cells.max()))
        run["group_profiles_ms_median"], run["group_profiles_ms_min"] = timed(
            lambda: _engine.group_profiles(dm, rows, group_ptr, shift))

        code = codes.astype(np.int32)
        for _ in range(2):
            _engine.rank_tables(dm, code, n_cells)
        samples, info = {name: [] for name in _engine.RANK_STAGES}, {}
        for _ in range(a.reps):
            ms = {}
            _engine.rank_tables(dm, code, n_cells, stage_ms=ms, info=info)
            for name in _engine.RANK_STAGES:
                samples[name].append(ms.get(name, 0.0))
        run["stage_ms_median"] = {k: statistics.median(v) for k, v in samples.items()}
        run["stage_ms_min"] = {k: min(v) for k, v in samples.items()}
        run["n_entries"], run["n_tiles"] = info["n_entries"], info["n_tiles"]
        run["tables_ms_median"], run["tables_ms_min"] = clocked(lambda: _engine.rank_tables(dm, code, n_cells))

        ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obs=pd.DataFrame({"clone": pd.Categorical(codes)}))
        ad.obsm["X_cnv"] = packed
        ad.uns["cnv"] = {"chr_pos": chr_pos}
        run["call_ms_median"], run["call_ms_min"] = clocked(lambda: cnv.tl.cnv_rank_groups(ad, "clone"), reps=3)
        _, call_info = cnv.tl.cnv_rank_groups(ad, "clone", return_info=True)
        run["call_stage_ms"] = call_info["stage_ms"]
        run["regions"] = int(len(ad.uns["cnv_rank_groups"]["regions"]))
        print(json.dumps(run), flush=True)

        # ---- the host baseline and the comparison, on the first --host-cells cells ------------------------------------------
        h = min(a.host_cells, n)
        if h > 0:
            sub = packed.dense_rows()[:h].to(torch.float64).cpu().numpy()
            t0 = time.perf_counter()
            ranks = scipy.stats.rankdata(sub, method="average", axis=0)
            t1 = time.perf_counter()
            onehot = scipy.sparse.csr_matrix((np.ones(h), (codes[:h], np.arange(h))), shape=(G, h))
            sums = np.asarray(onehot @ ranks)  # (half-integers below 2^53: the sums are exact in any order)
            t2 = time.perf_counter()
            run["host_cells"], run["host_rankdata_ms"], run["host_group_sums_ms"] = h, (t1 - t0) * 1e3, (t2 - t1) * 1e3
            sub_code = np.where(np.arange(n) < h, code, -1).astype(np.int32)
            r2, _, _ = _engine.rank_tables(dm, sub_code, np.bincount(codes[:h], minlength=G).astype(np.int64))
            run["host_equals_device"] = bool((np.rint(2.0 * sums).astype(np.int64) == r2.cpu().numpy()).all())
            del sub, ranks
            print(json.dumps({k: run[k] for k in ("host_cells", "host_rankdata_ms", "host_group_sums_ms",
                                                  "host_equals_device")}), flush=True)
        out["runs"].append(run)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Times of tl.cnv_kmeans's kernels at n = 20 000 and 100 000 cells x 50 float32 components with k = 6 and
64, HBM-resident as tl.pca leaves X_cnv_pca; the cells are k planted blobs (centres normal(0, 3), noise 1).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/microbench_ops.bin tools/microbench_ops.hip
    python tools/time_kmeans.py [--cells 20000 100000] [--components 50] [--clusters 6 64] [--reps 20]
                                [--ops-bin tools/microbench_ops.bin] [--sklearn-cells 20000] [--out profiles/time_kmeans.jsonl]

Per (n, k): device-event times (median and minimum over --reps launches after a warm-up) of icv_kmeans_assign, of
icv_kmeans_update with icv_kmeans_centres, and of one seeding (k draws: k - 1 icv_kmeans_seed_dist and k
icv_kmeans_seed_pick); the host-clock time of the public call (n_init = 10) on device input with its iterations.  The
instruction floor of the assignment is n x k x C x 3 float64 operations (a subtraction, a multiply, an add) at the issue
rate of v_add_f64 / v_mul_f64 that tools/microbench_ops.bin measures in the same run (cycles per wave-instruction per SIMD at
4 wavefronts per SIMD), at the nominal 2.4 GHz; without the binary the floor is left out and the line says so.  The
in-house yardstick for a float64 distance block, icv_silhouette_sums at --sklearn-cells cells and 6 groups, is timed in the
same run.  With scikit-learn present, ``sklearn.cluster.KMeans(n_init=10)`` on the host CPUs at --sklearn-cells cells,
labelled as such, with both inertias.  One JSON line per (n, k) is appended to --out."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_silhouette import NOMINAL_HZ, valu_f64_cycles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--clusters", type=int, nargs="+", default=[6, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ops-bin", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "microbench_ops.bin"))
    ap.add_argument("--sklearn-cells", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "time_kmeans.jsonl"))
    a = ap.parse_args()

    cycles = valu_f64_cycles(a.ops_bin)

    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib
    from infercnvpy_amd._compat import SimpleAnnData
    from infercnvpy_amd.tl import _kmeans
    from infercnvpy_amd.tl._groups import group_table
    from infercnvpy_amd.tl._silhouette import distance_shift

    lib = _lib.load()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rate = n_cu * 4 * 64 / cycles * NOMINAL_HZ if cycles else None
    print(f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; v_add_f64 / v_mul_f64: "
          + (f"{cycles:.2f} cycles per wave-instruction per SIMD = {rate / 1e12:.2f} T operations/s at 2.4 GHz"
             if cycles else "NOT MEASURED (no microbench_ops.bin): no instruction floor"), flush=True)
    ptr, st = _engine._ptr, _engine._stream_ptr(torch)

    def timed(launch):
        """(median, minimum) milliseconds of ``launch()`` by device events."""
        for _ in range(2):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(float(e0.elapsed_time(e1)))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms)}

    c = a.components
    for n in a.cells:
        for k in a.clusters:
            rng = np.random.default_rng(n + k)
            truth = rng.integers(0, k, n)
            x = (rng.normal(0, 3, (k, c))[truth] + rng.normal(0, 1, (n, c))).astype(np.float32)
            d_x = torch.from_numpy(x).cuda()
            e, f = _kmeans.shifts(float(np.abs(x).max()), n, c)
            head = (ptr(d_x), _lib.ICV_F32, n, c, c)
            centres = torch.zeros((k, c), dtype=torch.float64, device="cuda")
            labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            sqdist = torch.empty(n, dtype=torch.float64, device="cuda")
            state = torch.zeros(3, dtype=torch.int64, device="cuda")
            flags = state[2:].view(torch.int32)
            sums = torch.empty(k * (c + 1), dtype=torch.int64, device="cuda")
            mind = torch.empty(n, dtype=torch.float64, device="cuda")
            w = torch.empty(n, dtype=torch.int64, device="cuda")
            partials = torch.empty(-(-n // _lib.ICV_KMEANS_SEED_ROWS), dtype=torch.int64, device="cuda")
            picks = torch.empty(k, dtype=torch.int64, device="cuda")
            z = _kmeans.draws(0, 1, k)[0]

            def seeding():
                for t in range(k):
                    if t:
                        _lib.check(lib.icv_kmeans_seed_dist(*head, C.c_void_p(centres.data_ptr() + 8 * c * (t - 1)), int(t == 1),
                                                            f, ptr(mind), ptr(w), ptr(partials), ptr(flags), st))
                    _lib.check(lib.icv_kmeans_seed_pick(*head, ptr(w) if t else None, ptr(partials) if t else None, t, k, z[t],
                                                        ptr(centres), ptr(picks), ptr(flags), st))

            def assign():
                _lib.check(lib.icv_kmeans_assign(*head, ptr(centres), k, f, ptr(labels), ptr(sqdist), ptr(state), ptr(flags), st))

            def update():
                _lib.check(lib.icv_kmeans_update(*head, ptr(labels), k, e, ptr(sums), st))
                _lib.check(lib.icv_kmeans_centres(ptr(sums), k, c, e, ptr(centres), st))

            out = {"cells": n, "components": c, "clusters": k, "dtype": "float32", "shift": [e, f], "reps": a.reps,
                   "device": torch.cuda.get_device_name(0)}
            out["seeding"] = timed(seeding)
            out["assign"] = timed(assign)  # (the centres are the seeded rows; the labels settle in the warm-up)
            out["update"] = timed(update)
            assert int(state[2].item()) == 0
            ops = float(n) * k * c * 3.0
            out["float64_operations"] = ops
            if rate:
                out["valu_f64_cycles_per_wave_instruction"] = cycles
                out["floor_ms_at_2.4GHz"] = ops / rate * 1e3
                out["fraction_of_floor"] = out["floor_ms_at_2.4GHz"] / out["assign"]["ms_median"]
            else:
                out["floor_ms_at_2.4GHz"] = None
            ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32))
            ad.obsm["X_cnv_pca"] = d_x
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                _, _, info = cnv.tl.cnv_kmeans(ad, k, n_init=10, return_info=True)
                t.append((time.perf_counter() - t0) * 1e3)
            out["public_call_ms"] = {"median": statistics.median(t), "min": min(t)}
            out["public_call_iterations"] = [len(run) for run in info["history"]]
            out["public_call_stage_ms"] = info["stage_ms"]
            out["inertia"] = ad.uns["cnv_kmeans"]["inertia"]
            if n == a.sklearn_cells:
                if k == a.clusters[0]:  # the yardstick: the silhouette's distance block at the same cells, 6 groups
                    codes = rng.integers(0, 6, size=n).astype(np.int64)
                    rows, group_ptr, sizes = group_table(codes, 6)
                    shift, dist_exp = distance_shift(float(np.abs(x).max()), int(sizes.max()), c)
                    dm = _engine.matrix_input(d_x, "time_kmeans")
                    for _ in range(2):
                        _engine.silhouette(dm, rows, group_ptr, shift, dist_exp)
                    got = []
                    for _ in range(a.reps):
                        ms = {}
                        _engine.silhouette(dm, rows, group_ptr, shift, dist_exp, stage_ms=ms)
                        got.append(ms["sums"])
                    out["silhouette_sums_ms_median"] = statistics.median(got)
                    if rate:
                        out["silhouette_fraction_of_floor"] = float(n) * n * c * 3.0 / rate * 1e3 / statistics.median(got)
                try:
                    from sklearn.cluster import KMeans
                except ImportError:
                    out["sklearn_host_ms"] = None  # (not measured: scikit-learn is not installed)
                else:
                    t0 = time.perf_counter()
                    theirs = KMeans(n_clusters=k, n_init=10, random_state=0).fit(x.astype(np.float64))
                    out["sklearn_host_ms"] = (time.perf_counter() - t0) * 1e3
                    out["sklearn_host_cpus"] = len(os.sched_getaffinity(0))
                    out["sklearn_inertia"] = float(theirs.inertia_)
            print(json.dumps(out), flush=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(out) + "\n")
            del d_x
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Times of tl.cnv_silhouette's kernels at n = 20 000 and 100 000 cells x 50 float32 components with 6 and
500 groups of random labels, HBM-resident as tl.pca leaves X_cnv_pca.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/microbench_ops.bin tools/microbench_ops.hip
    python tools/time_silhouette.py [--cells 20000 100000] [--components 50] [--groups 6 500] [--reps 20]
                                    [--ops-bin tools/microbench_ops.bin] [--sklearn-cells 20000] [--out profiles/time_silhouette.jsonl]

Per (n, G): device-event times (median and minimum over --reps launches after a warm-up) of icv_silhouette_sums and
icv_silhouette_finish, of the sums on the same cells times 2^13 where that makes the rounding rint and a conversion instead
of one addition (groups below 512 cells), and the host-clock time of the public call on device input.  The instruction floor of the sums is
n^2 ordered pairs x C x 3 float64 operations (a subtraction, a multiply, an add) at the issue rate of v_add_f64 /
v_mul_f64 that tools/microbench_ops.bin measures in the same run (cycles per wave-instruction per SIMD at 4 wavefronts
per SIMD, the kernel's occupancy), at the nominal 2.4 GHz: the clock under load is lower, so the fraction reached is a
lower bound.  Without the binary the floor is left out and the line says so.  With scikit-learn present,
``sklearn.metrics.silhouette_samples`` on the host CPUs at --sklearn-cells cells, labelled as such, and the largest
difference from it.  One JSON line per (n, G) is appended to --out."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NOMINAL_HZ = 2.4e9


def valu_f64_cycles(ops_bin):
    """Cycles per v_add_f64 / v_mul_f64 wave-instruction per SIMD at 4 wavefronts per SIMD, from the microbenchmark's
    output (a child process of its own, before this one opens the GPU); None without the binary."""
    if not ops_bin or not os.path.exists(ops_bin):
        return None
    out = subprocess.run([ops_bin], capture_output=True, text=True, timeout=120, check=True).stdout
    found = {}
    for name in ("v_add_f64", "v_mul_f64"):
        m = re.search(rf"^{name}\s.*4 w/SIMD:\s*([0-9.]+)", out, re.M)
        if m:
            found[name] = float(m.group(1))
    return max(found.values()) if len(found) == 2 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--groups", type=int, nargs="+", default=[6, 500])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ops-bin", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "microbench_ops.bin"))
    ap.add_argument("--sklearn-cells", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "time_silhouette.jsonl"))
    a = ap.parse_args()

    cycles = valu_f64_cycles(a.ops_bin)

    import pandas as pd
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine
    from infercnvpy_amd._compat import SimpleAnnData
    from infercnvpy_amd.tl._groups import group_table
    from infercnvpy_amd.tl._silhouette import distance_shift

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    # float64 operations per second of the whole chip at the measured issue rate and the nominal clock
    rate = n_cu * 4 * 64 / cycles * NOMINAL_HZ if cycles else None
    print(f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; v_add_f64 / v_mul_f64: "
          + (f"{cycles:.2f} cycles per wave-instruction per SIMD = {rate / 1e12:.2f} T operations/s at 2.4 GHz"
             if cycles else "NOT MEASURED (no microbench_ops.bin): no instruction floor"), flush=True)

    def stage_times(dm, rows, group_ptr, shift, dist_exp):
        for _ in range(2):
            _engine.silhouette(dm, rows, group_ptr, shift, dist_exp)
        torch.cuda.synchronize()
        sums, finish = [], []
        for _ in range(a.reps):
            ms = {}
            _engine.silhouette(dm, rows, group_ptr, shift, dist_exp, stage_ms=ms)
            sums.append(ms["sums"])
            finish.append(ms["finish"])
        return sums, finish

    c = a.components
    for n in a.cells:
        rng = np.random.default_rng(n)
        x = rng.normal(0.0, 1.0, (n, c)).astype(np.float32)
        d_x = torch.from_numpy(x).cuda()
        dm = _engine.matrix_input(d_x, "time_silhouette")
        for g in a.groups:
            codes = rng.integers(0, g, size=n).astype(np.int64)
            sizes = np.bincount(codes, minlength=g)
            rows, group_ptr, _ = group_table(codes, g)
            shift, dist_exp = distance_shift(float(np.abs(x).max()), int(sizes.max()), c)
            sums, finish = stage_times(dm, rows, group_ptr, shift, dist_exp)
            out = {"cells": n, "components": c, "groups": g, "dtype": "float32", "shift": shift, "reps": a.reps,
                   "largest_group": int(sizes.max()), "j_tiles": int(_engine.silhouette_tiles(group_ptr, 1)[0].shape[1]),
                   "sums": {"ms_median": statistics.median(sums), "ms_min": min(sums)},
                   "finish": {"ms_median": statistics.median(finish), "ms_min": min(finish)},
                   "device": torch.cuda.get_device_name(0)}
            # the same cells times 2^13: with groups below 512 cells d 2^e reaches 2^51 there, so the rounding is rint and a
            # conversion, not one addition (larger groups lower e instead and keep the addition)
            shift_b, exp_b = distance_shift(float(np.abs(x).max()) * 8192.0, int(sizes.max()), c)
            if shift_b + exp_b > 51 >= shift + dist_exp:
                big = _engine.matrix_input(d_x * 8192.0, "time_silhouette")
                sums_b, _ = stage_times(big, rows, group_ptr, shift_b, exp_b)
                out["sums_rint_form"] = {"ms_median": statistics.median(sums_b), "ms_min": min(sums_b), "shift": shift_b}
                del big
            ops = float(n) * float(n) * c * 3.0
            out["float64_operations"] = ops
            if rate:
                out["valu_f64_cycles_per_wave_instruction"] = cycles
                out["floor_ms_at_2.4GHz"] = ops / rate * 1e3
                out["fraction_of_floor"] = out["floor_ms_at_2.4GHz"] / out["sums"]["ms_median"]
            else:
                out["floor_ms_at_2.4GHz"] = None
            ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obs=pd.DataFrame({"clone": pd.Categorical(codes)}))
            ad.obsm["X_cnv_pca"] = d_x
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                cnv.tl.cnv_silhouette(ad, "clone")
                t.append((time.perf_counter() - t0) * 1e3)
            out["public_call_ms"] = {"median": statistics.median(t), "min": min(t)}
            if n == a.sklearn_cells:
                try:
                    from sklearn.metrics import silhouette_samples
                except ImportError:
                    out["sklearn_host_ms"] = None  # (not measured: scikit-learn is not installed)
                else:
                    t0 = time.perf_counter()
                    theirs = silhouette_samples(x.astype(np.float64), codes)
                    out["sklearn_host_ms"] = (time.perf_counter() - t0) * 1e3
                    out["sklearn_host_cpus"] = len(os.sched_getaffinity(0))
                    out["sklearn_largest_difference"] = float(np.abs(ad.obs["cnv_silhouette"].to_numpy() - theirs).max())
            print(json.dumps(out), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(out) + "\n")
        del dm, d_x
    return 0


if __name__ == "__main__":
    sys.exit(main())

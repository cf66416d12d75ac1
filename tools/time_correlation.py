"""Times of tl.cnv_correlation's kernel at the geometry of the tl.cnv_states figures (100 000 cells x 1 802 windows, 13 %
stored, float64 CSR, HBM-resident as tl.infercnv leaves it).

    python tools/time_correlation.py [--cells 100000] [--windows 1802] [--density 0.13] [--groups 0 1 6 500] [--reps 20]
                                     [--host-groups 6 500]

Device-event times (median and minimum over --reps launches after a warm-up) of icv_profile_corr for every G of --groups
on the CSR input and for G = 6 on the dense float32 form, of icv_profile_corr_best, and in the same run of the two
yardsticks that read the same 12 bytes per stored entry, icv_group_profiles (6 groups) and icv_states_viterbi; the copy
rate of HBM measured in the same run; the host-clock time of the public calls on device input; and the host baseline
``scipy.sparse @ profiles.T`` plus the numpy finish on the CPUs of the box.  The result is checked against that
baseline."""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--groups", type=int, nargs="+", default=[0, 1, 6, 500])
    ap.add_argument("--host-groups", type=int, nargs="*", default=[6, 500])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import pandas as pd
    import scipy.sparse as sp
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib
    from infercnvpy_amd._compat import SimpleAnnData
    from infercnvpy_amd.tl._correlation import centre_profiles
    from infercnvpy_amd.tl._pseudobulk import profile_shift
    from time_pca import synthetic_packed
    from time_states import chromosome_bounds

    n, w = a.cells, a.windows
    packed = synthetic_packed(n, w, a.density)
    nnz = packed.nnz()
    dm = _engine.matrix_input(packed, "time_correlation")
    dense32 = packed.dense_rows().contiguous()  # (the device float32 n x W form of the same matrix)
    dm32 = _engine.matrix_input(dense32, "time_correlation")
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

    print(f"device: {torch.cuda.get_device_name(0)}; {n} cells x {w} windows, {nnz} stored ({nnz / (n * w):.3f}), "
          f"median / minimum of {a.reps} launches, device events", flush=True)
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()  # 1 GiB read and 1 GiB written
    dst = torch.empty_like(src)
    copy_ms, _ = timed(lambda: dst.copy_(src))
    hbm = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e12
    del src, dst
    print(f"HBM copy rate of this run: {hbm:.2f} TB/s", flush=True)
    csr_bytes, dense_bytes = 12 * nnz + 16 * n, 4 * n * w

    # ---- the yardsticks: the same 12 bytes per stored entry ----------------------------------------------------------------
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 6, size=n)
    rows = torch.from_numpy(np.argsort(codes, kind="stable").astype(np.int64)).cuda()
    sizes = np.bincount(codes, minlength=6)
    group_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).cuda()
    shift = profile_shift(int(sizes.max()))
    gp_ms, gp_min = timed(lambda: _engine.group_profiles(dm, rows, group_ptr, shift))
    q, flag = _engine.states_rowsq(dm)
    sigma = math.sqrt(math.fsum(q.cpu().numpy().tolist()) / (float(n) * float(w)))
    bounds = chromosome_bounds(w)
    cs = torch.from_numpy(bounds).cuda()
    states = torch.empty((n, w), dtype=torch.int8, device="cuda")
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    m = dm.c_struct()

    def viterbi():
        _lib.check(lib.icv_states_viterbi(C.byref(m), _engine._ptr(cs), int(bounds.shape[0]) - 1, 2.0 * sigma,
                                          1.0 / (2.0 * sigma * sigma), math.log(1.0 - 1e-3), math.log(1e-3 / 2.0),
                                          _engine._ptr(states), _engine._ptr(count), st))

    vt_ms, vt_min = timed(viterbi)
    rq_ms, rq_min = timed(lambda: _engine.states_rowsq(dm))
    del states
    print(f"yardstick icv_group_profiles (6 groups): {gp_ms:.3f} / {gp_min:.3f} ms "
          f"({csr_bytes / (gp_ms * 1e-3) / 1e12:.2f} TB/s of matrix bytes)")
    print(f"yardstick icv_states_viterbi:            {vt_ms:.3f} / {vt_min:.3f} ms")
    print(f"yardstick icv_states_rowsq:              {rq_ms:.3f} / {rq_min:.3f} ms", flush=True)

    # ---- icv_profile_corr ------------------------------------------------------------------------------------------------------
    results = {}
    for form, mat, nbytes, groups in (("csr_float64", dm, csr_bytes, a.groups), ("dense_float32", dm32, dense_bytes, [6])):
        for g in groups:
            p = rng.normal(0.0, 0.1, (g, w))
            c, s2 = centre_profiles(p) if g else (None, None)
            out = _engine.profile_corr(mat, c, s2)
            ms, lo = timed(lambda: _engine.profile_corr(mat, c, s2))
            best_ms, _ = timed(lambda: _engine.profile_corr_best(out[3]))
            results[(form, g)] = (p, out)
            print(f"icv_profile_corr {form} G={g:<4d}: {ms:.3f} / {lo:.3f} ms = {ms / gp_ms:.2f} x group_profiles, "
                  f"{ms / vt_ms:.2f} x viterbi; {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s of matrix bytes "
                  f"({nbytes / (ms * 1e-3) / 1e12 / hbm:.2f} of the copy rate), "
                  f"{2.0 * nnz * g / (ms * 1e-3) / 1e12 if form.startswith('csr') else 2.0 * n * w * g / (ms * 1e-3) / 1e12:.2f} "
                  f"TFLOP/s in D; icv_profile_corr_best {best_ms:.3f} ms", flush=True)

    # ---- the public calls on device input --------------------------------------------------------------------------------------
    ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obs=pd.DataFrame({"clone": pd.Categorical(codes)}))
    ad.obsm["X_cnv"] = packed
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0}}
    for name, fn in (("tl.cnv_signal", lambda: cnv.tl.cnv_signal(ad)),
                     ("tl.cnv_correlation (top 5 %)", lambda: cnv.tl.cnv_correlation(ad)),
                     ("tl.cnv_correlation (groupby, 6 groups)", lambda: cnv.tl.cnv_correlation(ad, groupby="clone"))):
        ms, lo = clocked(fn)
        print(f"public call {name}: {ms:.2f} / {lo:.2f} ms (host clock)", flush=True)

    # ---- the host baseline -----------------------------------------------------------------------------------------------------
    host = sp.csr_matrix((packed.data[:nnz].cpu().numpy(), packed.indices[:nnz].cpu().numpy(), packed.indptr.cpu().numpy()),
                         shape=(n, w))
    for g in a.host_groups:
        if ("csr_float64", g) not in results:
            continue
        p, out = results[("csr_float64", g)]

        def baseline():
            c = p - p.mean(axis=1, keepdims=True)
            d = host @ c.T
            s = np.asarray(host.sum(axis=1)).ravel()
            b = np.asarray(host.multiply(host).sum(axis=1)).ravel()
            vx = b - s * s / w
            with np.errstate(all="ignore"):
                return np.clip(d / np.sqrt(vx[:, None] * (c * c).sum(axis=1)[None, :]), -1.0, 1.0)

        t = []
        for _ in range(3 if g <= 64 else 1):
            t0 = time.perf_counter()
            ref = baseline()
            t.append((time.perf_counter() - t0) * 1e3)
        diff = float(np.nanmax(np.abs(out[3].cpu().numpy() - ref)))
        print(f"host baseline scipy.sparse @ profiles.T + numpy finish, G={g}: {statistics.median(t):.1f} ms "
              f"({os.cpu_count()} CPUs seen, {len(os.sched_getaffinity(0))} usable); largest |r - baseline| = {diff:.3g}",
              flush=True)


if __name__ == "__main__":
    main()

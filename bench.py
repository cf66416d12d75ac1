#!/usr/bin/env python
"""Benchmark of the tl.infercnv hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

With N > 1 and no WORLD_SIZE in the environment the script re-executes itself as
``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...`` (one rank per
GPU, backend nccl = RCCL over xGMI); it exits non-zero if the box has fewer than N GPUs.  Started by a launcher
(WORLD_SIZE set) it checks that WORLD_SIZE == --gpus.

One "step" = one pass of the whole hot path over one batch of synthetic cells that is already resident in HBM.
  N = 1   ONE CALL OF THE PUBLIC FUNCTION, cnv.tl.infercnv(adata) with the reference's default arguments
          (reference=None: the all-cell mean is part of the step), on BASELINE config 2: dense fp32 100 000 cells x
          20 000 genes (chr1..22, random var order) as a CUDA tensor in adata.X, window 100, step 10, chunksize 5000.
          Inside: reference-order column means (k_colchain, bit-equal to np.mean) -> fused centre / clip /
          pyramid-smooth / median kernel -> per-chunk std -> noise threshold + CSR packing of X_cnv
          (k_thr_mask_ring, k_row_offsets, k_csr_fill_ring; reference _infercnv.py:449-455 is inside the chunk kernel)
          -> X_cnv as device CSR float64.
          The calls are issued back to back without host synchronisation (the function does not wait for the GPU).
  N > 1   one process per GPU over the rows of config 3 (dist.run_shard per rank).  THREE forms of the reference means
          are timed back to back, K steps each.  Two give the reference's own bits (X_cnv bit-identical to the N = 1
          public call for any N): `value_blocks_means` -- the ranks' passes CONCURRENT, the float32 chain by integer
          blocks (dist.reference_means_blocks: float64 totals, ONE all-gather of [G] float64, block records on every rank
          at once, a scan over the records from rank to rank, means broadcast) -- and `value_chained_means` -- the
          icv_colchain accumulators handed from rank to rank (dist.reference_means_chained: the ranks take turns, pipelined
          over two column groups).  `value` = the FASTER of those two at this N (the blocks pay two passes over a rank's
          rows and win from ~4 ranks on; dist.reference_means_exact chooses alike);
          `value_allreduce_means` = float64 column sums + ONE RCCL all-reduce of [G + 1] float64 (concurrent, correctly
          rounded means -- not the reference's bits: tl.infercnv(mean_order="float64")).  All -> the same smoothing kernel ->
          per-chunk std -> noise threshold + CSR pack (dist.run_shard(pack=True)).
          The N = 1 line carries `scale_n1`: config 3's 1 M cells on ONE rank through this same per-rank code path,
          both forms -- the N = 1 point a scaling curve over the N > 1 lines starts from.
  N > 1   BASELINE config 3: 1 000 000 cells x 20 000 genes in total, row shards aligned to the 5000-cell chunks
          (dist.shard_bounds; 125 000 cells per GPU at N = 8): strong scaling.  Every 5000-cell chunk is generated
          from its own seed, so the data do not depend on N.

Prints ONE JSON line on rank 0: value = cells/s of the whole job (HBM-resident input), ms_per_step = the
milliseconds of one timed step (--steps of them after --warmup untimed ones), plus
  roofline     - the smoothing kernel: algorithmic bytes (4*G + 4*W per cell) / its average HIP-event duration
                 (events recorded by the library on the launch stream during the timed steps), against the 8 TB/s
                 HBM peak
A plain run stops there.  With ``--full`` the line also carries the figures that take runs of their own:
  cpu_baseline - the numpy oracle (a port of the reference algorithm, oracle/) on this box's host cores on a
                 bounded sample of the same workload (rank 0, N = 1 only)
  e2e          - the public cnv.tl.infercnv(adata) from HOST memory to a host CSR X_cnv (PCIe-inclusive, rank 0).
                 N = 1: dense 200 000 x 20 000 and the config-4 CSR.  N > 1: ONE call with devices=[0..N-1] (the
                 multi-GPU path of the public API: row shards, one uploader + CSR drain per GPU), 100 000 dense
                 cells per GPU, while the other ranks wait at a barrier with their HBM released.
  stages       - (N = 1) the step's kernels timed one by one with events on the launch stream (engine-level calls that
                 mirror the public function), each with its own roofline: k_colchain, smoothing + thresholds, threshold + CSR pack
  extra        - (N = 1) the other BASELINE configurations, HBM resident, through the same public call, each with its
                 own roofline: config 4 (CSR window 250), CSR window 100, config 3's 1 M cells on one GPU, the round-3
                 form of the step (float64 column sums + in-place threshold, no CSR), config 5 (distances + Ward at
                 200 000 x 5 000 when HBM allows).
  (N > 1)      - value_allreduce_means: the float64 all-reduce form of the means, timed after the two exact forms.

``--dump-outputs DIR``: after the timed steps, X_cnv of the last step as float64 .npy files in DIR (a seeded sample
of its rows, per-row sums and entry counts, chr_pos; see dump_outputs).  The inputs are generated from fixed seeds, so
two builds run with the same arguments can be compared output for output.

``--dry-run-one-gpu`` (never a measurement: prints "dry_run": true): all N ranks share cuda:0 and the collectives
go through gloo -- exercises the launcher, the sharding and the N > 1 code paths on a one-GPU box.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3  # same guide: dense fp32 MFMA peak
CHUNK = 5000


class _OncePerProcess:
    """logging filter: a message of the library that repeats on every call (the reference's "Using mean of all cells as
    reference" warning, once per tl.infercnv call = several hundred times per bench run) is shown ONCE -- the record
    of a driver run is the tail of this process's output, and VERDICT r5 found nothing but that warning in it.  A
    filter on the bench process's logger, not a product change."""

    def __init__(self):
        self.seen = set()

    def filter(self, record):
        key = str(record.msg)[:60]
        if key in self.seen:
            return False
        self.seen.add(key)
        return True


def quiet_repeated_warnings():
    import logging

    logging.getLogger("infercnvpy_amd").addFilter(_OncePerProcess())


CONFIG2_CELLS = 100_000
CONFIG3_CELLS = 1_000_000
G = 20000


def synth_chunk(torch, n_rows, n_genes, seed):
    """gamma(0.3, 1) with entries < 0.5 zeroed (~19 % nnz), SURVEY §8(d) config 2 -- generated on the GPU."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    g = torch._standard_gamma(torch.full((n_rows, n_genes), 0.3, device="cuda"), generator=gen)
    return torch.where(g < 0.5, torch.zeros_like(g), g)


def synth_rows(torch, row0, row1, n_genes, chunk=CHUNK, seed0=2):
    """Rows [row0, row1) of the synthetic matrix; chunk k (rows k*chunk ...) has seed seed0 + k."""
    out = torch.empty((row1 - row0, n_genes), dtype=torch.float32, device="cuda")
    r = row0
    while r < row1:
        k = r // chunk
        blk = synth_chunk(torch, chunk, n_genes, seed0 + k)
        a, b = r - k * chunk, min(row1, (k + 1) * chunk) - k * chunk
        out[r - row0: r - row0 + (b - a)] = blk[a:b]
        r += b - a
    return out


def synth_csr_on_device(torch, n_cells, n_genes, density, seed):
    """10x-like CSR: Bernoulli(density) mask x log1p(1 + poisson-ish counts)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    indptr = [torch.zeros(1, dtype=torch.int64, device="cuda")]
    indices, data = [], []
    rows, nnz = 10_000, 0
    for r in range(0, n_cells, rows):
        k = min(rows, n_cells - r)
        mask = torch.rand((k, n_genes), device="cuda", generator=gen) < density
        vals = torch.log1p(1.0 + torch.floor(torch.rand((k, n_genes), device="cuda", generator=gen) ** 3 * 8.0))
        counts = mask.sum(dim=1)
        indptr.append(nnz + torch.cumsum(counts, 0))
        nnz += int(counts.sum())
        idx = mask.nonzero(as_tuple=False)
        indices.append(idx[:, 1].to(torch.int32))
        data.append(vals[mask].float())
    return torch.cat(indptr), torch.cat(indices), torch.cat(data)


# ----------------------------------------------------------------------------------------------------------
# CPU baseline: the oracle's chunk kernel, one worker per host core; every worker generates its own chunk, so
# the number is compute only (no pickling of the matrix through the pool feeder)
# ----------------------------------------------------------------------------------------------------------
def _cpu_worker(args):
    import numpy as np

    import cases
    from oracle import infercnv_oracle as O

    seed, n_cells, window, step, reps = args
    v = cases.synthetic_var(cases.GENES_PER_CHROM_20K)
    X = cases.synthetic_expr(n_cells, 20000, seed=seed)
    ref = X.mean(axis=0, dtype=np.float64).astype(np.float32)[None, :]
    t0 = time.perf_counter()
    for _ in range(reps):
        O.infercnv_chunk(X, v["chromosome"], v["start"], ref, 3, window, step, 1.5)
    return time.perf_counter() - t0


def _physical_cores():
    """Physical cores of the box (distinct (package, core) pairs in /proc/cpuinfo); logical count if unknown."""
    try:
        seen, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        return len(seen) or (os.cpu_count() or 1)
    except OSError:
        return os.cpu_count() or 1


def _cpu_pool(workers):
    """Process pool of the CPU baseline.  The workers are spawned, not forked: this process has the GPU open, and
    forked children would inherit its device handles."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor

    return ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn"))


def _cpu_pool_rate(workers, window, step, cells_per_worker, reps):
    tasks = [(100 + i, cells_per_worker, window, step, reps) for i in range(workers)]
    t0 = time.perf_counter()
    with _cpu_pool(workers) as pool:
        busy = list(pool.map(_cpu_worker, tasks))
    wall = time.perf_counter() - t0
    n = cells_per_worker * workers * reps
    # all workers run concurrently: throughput = cells / the slowest worker's compute time
    return n / max(busy), n, max(busy), wall


def _cpu_chunk_worker(args):
    """One 5000-cell chunk as the reference's process pool runs it (one task = one chunk, tl/_infercnv.py:120-135)."""
    import numpy as np

    import cases
    from oracle import infercnv_oracle as O

    seed, n_cells, window, step = args
    v = cases.synthetic_var(cases.GENES_PER_CHROM_20K)
    X = cases.synthetic_expr(n_cells, 20000, seed=seed)
    ref = X.mean(axis=0, dtype=np.float64).astype(np.float32)[None, :]
    t0 = time.perf_counter()
    O.infercnv_chunk(X, v["chromosome"], v["start"], ref, 3, window, step, 1.5)
    return time.perf_counter() - t0


def cpu_baseline(window=100, step=10, cells_per_worker=400, reps=2, slice_cells=100_000, chunk=CHUNK):
    logical = os.cpu_count() or 1
    physical = min(_physical_cores(), logical)
    # the reference's structure -- ProcessPoolExecutor over 5000-row chunks of a 100 000-cell slice (20
    # tasks), one worker per physical core; every worker builds its own chunk (the matrix is not pickled through the
    # pool), the clock runs over the slowest chunk's compute time and, separately, over the wall time of the pool
    n_tasks = slice_cells // chunk
    t0 = time.perf_counter()
    with _cpu_pool(min(physical, n_tasks)) as pool:
        busy = list(pool.map(_cpu_chunk_worker, [(300 + i, chunk, window, step) for i in range(n_tasks)]))
    wall = time.perf_counter() - t0
    spec = {
        "value": slice_cells / max(busy), "unit": "cells/s", "cores": min(physical, n_tasks), "kind": "port",
        "wall_cells_per_s": slice_cells / wall, "per_process_cells_per_s": chunk / (sum(busy) / len(busy)),
        "sample": f"SURVEY 8(d): {n_tasks} chunks of {chunk} cells (a {slice_cells}-cell slice of config 2: dense fp32 x "
                  f"20000 genes, window {window} step {step}) through ProcessPoolExecutor(max_workers={min(physical, n_tasks)} "
                  f"of {physical} physical cores), oracle chunk kernel (per-row np.convolve as the reference); slowest "
                  f"chunk {max(busy):.1f} s, mean {sum(busy) / len(busy):.1f} s, pool wall {wall:.1f} s incl. start-up and "
                  f"building the chunks",
    }
    out = dict(spec)
    # the whole box on config 3's chunk list: 200 chunks of 5000 cells (1 M cells) through one pool of min(physical
    # cores, 200) workers, the reference's own structure at its default n_jobs (process_map(max_workers=cpu_count()),
    # tl/_infercnv.py:120-135); the rate is cells / pool wall time after the workers have built their chunks (the clock
    # of every chunk runs over its compute only; wall = the pool's makespan of those compute times, reconstructed from
    # the per-chunk times in task order over `workers` slots)
    n_cfg3 = CONFIG3_CELLS // chunk
    workers = max(1, min(physical, n_cfg3))
    t0 = time.perf_counter()
    with _cpu_pool(workers) as pool:
        busy3 = list(pool.map(_cpu_chunk_worker, [(700 + i, chunk, window, step) for i in range(n_cfg3)]))
    wall3 = time.perf_counter() - t0
    slots = [0.0] * workers
    for b in busy3:  # greedy list scheduling in task order = what the pool does
        k = slots.index(min(slots))
        slots[k] += b
    makespan = max(slots)
    out["whole_box"] = {
        "value": n_cfg3 * chunk / makespan, "unit": "cells/s", "cores": workers, "kind": "port",
        "wall_cells_per_s": n_cfg3 * chunk / wall3, "per_process_cells_per_s": chunk / (sum(busy3) / len(busy3)),
        "sample": f"config 3's chunk list: {n_cfg3} chunks of {chunk} cells (1 M cells x 20000 genes dense fp32, window "
                  f"{window} step {step}) through ProcessPoolExecutor(max_workers={workers} = min(physical cores "
                  f"{physical}, {n_cfg3})), oracle chunk kernel; makespan of the chunks' compute times {makespan:.1f} s "
                  f"(mean chunk {sum(busy3) / len(busy3):.1f} s, slowest {max(busy3):.1f} s), pool wall {wall3:.1f} s "
                  f"incl. start-up and building the chunks",
    }
    try:
        from infercnvpy_amd._engine import _usable_cpus

        usable = _usable_cpus()
    except Exception:
        usable = logical
    out["usable_cpus"] = usable
    out["usable_cpus_note"] = (f"logical CPUs {logical}, physical cores {physical}; the process may use {usable} CPUs of "
                               f"time (affinity mask / cgroup quota): pools with more workers than that share them")
    rate_l, n_l, busy_l, wall_l = _cpu_pool_rate(logical, window, step, cells_per_worker, reps)
    out["oversubscribed"] = {
        "value": rate_l, "unit": "cells/s", "cores": logical, "kind": "port",
        "per_process_cells_per_s": rate_l / logical,
        "sample": f"{logical} processes (one per logical CPU) x {reps} x {cells_per_worker}-cell chunks ({n_l} cells x "
                  f"20000 genes dense fp32, window {window} step {step}), oracle chunk kernel (per-row np.convolve as "
                  f"the reference) on worker-local data; slowest worker {busy_l:.1f} s compute, {wall_l:.1f} s wall "
                  f"incl. start-up.  {rate_l / logical:.0f} cells/s per process against ~600-900 for one process alone "
                  f"on an idle box: with every logical CPU busy the box is memory-bandwidth / SMT bound (each chunk "
                  f"pass streams ~0.5 GB through numpy temporaries), so this is the whole-box rate, not cores x the "
                  f"single-core rate",
    }
    return out


# ----------------------------------------------------------------------------------------------------------
# end to end through the public API, from host memory
# ----------------------------------------------------------------------------------------------------------
def _stage_seconds(tm):
    out = {}
    for k, x in tm.items():
        if isinstance(x, (int, float)) and k not in ("kernel",):
            out[k] = round(float(x), 4)
    return out


def _e2e_run(name, X, window, legs, devices=None, repeats=2, default_reference=False):
    import gc

    import numpy as np
    import pandas as pd
    import scipy.sparse as sp

    import cases
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    v = cases.synthetic_var(cases.GENES_PER_CHROM_20K)
    var = pd.DataFrame({"chromosome": v["chromosome"], "start": v["start"], "end": v["end"]}, index=v["names"])
    ref = np.asarray(X[:2000].mean(axis=0), dtype=np.float64).ravel().astype(np.float32)
    best, ad, all_dt = None, None, []
    for _ in range(repeats):  # first call pays one-time costs (pinned staging buffers, plan tables, contexts)
        ad = None  # a fresh AnnData per call: releasing the previous X_cnv (> 1 GB) is not part of the call
        gc.collect()
        ad = SimpleAnnData(X, var=var)
        tm = {}
        t0 = time.perf_counter()
        if default_reference:  # the reference's default call: the all-cell mean is formed on the GPU (reference order)
            cnv.tl.infercnv(ad, window_size=window, step=10, devices=devices, _timings=tm)
        else:
            cnv.tl.infercnv(ad, reference=ref, window_size=window, step=10, devices=devices, _timings=tm)
        dt = time.perf_counter() - t0
        all_dt.append(round(dt, 4))
        if best is None or dt < best[0]:
            best = (dt, tm)
    dt, tm = best
    in_bytes = X.data.nbytes + X.indices.nbytes + X.indptr.nbytes if sp.issparse(X) else X.nbytes
    legs[name] = {
        "cells": int(X.shape[0]), "seconds": dt, "cells_per_s": X.shape[0] / dt, "devices": tm.get("devices"),
        # per-GPU upload rate of the slowest shard's helper thread, and what all links moved together per second
        "h2d_GBps": in_bytes / max(len(tm.get("devices") or [0]), 1) / max(tm.get("h2d", dt), 1e-9) / 1e9,
        "h2d_GBps_all_gpus": in_bytes / max(tm.get("h2d", dt), 1e-9) / 1e9,
        "input_GB": in_bytes / 1e9,
        "x_cnv_nnz": int(ad.obsm["X_cnv"].nnz), "stages_s": _stage_seconds(tm),
        "seconds_every_repeat": all_dt,  # (the first one pays the one-time costs; `seconds` is the fastest)
    }
    if "shards" in tm:
        legs[name]["shards"] = tm["shards"]


def e2e_legs(torch, window_dense=100, dense_cells=200_000, csr_cells=500_000):
    import scipy.sparse as sp

    legs = {}
    only = os.environ.get("BENCH_E2E_LEGS", "dense,csr,1m").split(",")  # (debugging aid: a subset of the legs)
    if "dense" in only:
        Xd = synth_rows(torch, 0, dense_cells, G).cpu().numpy()
        _e2e_run(f"dense fp32 {dense_cells} x 20000, window {window_dense}", Xd, window_dense, legs, devices=[0], repeats=6)
        _e2e_run(f"dense fp32 {dense_cells} x 20000, window {window_dense}, reference=None (means on the GPU, in numpy's order)",
                 Xd, window_dense, legs, devices=[0], repeats=1, default_reference=True)
        del Xd
    if "csr" in only:
        ip, ix, dv = synth_csr_on_device(torch, csr_cells, G, 0.07, seed=3)
        Xs = sp.csr_matrix((dv.cpu().numpy(), ix.cpu().numpy(), ip.cpu().numpy()), shape=(csr_cells, G))
        del ip, ix, dv
        torch.cuda.empty_cache()
        _e2e_run(f"CSR fp32 {csr_cells} x 20000 density 0.07, window 250 (BASELINE config 4)", Xs, 250, legs, devices=[0])
        _e2e_run(f"CSR fp32 {csr_cells} x 20000 density 0.07, window 250, reference=None (means on the GPU, in scipy's order)",
                 Xs, 250, legs, devices=[0], repeats=1, default_reference=True)
        del Xs
    # north_star's own size from HOST memory (1 000 000 x 20 000 dense fp32 = 80 GB): only where the box has the RAM
    try:
        import psutil

        avail = psutil.virtual_memory().available
    except Exception:
        avail = 0
    if avail >= 130e9 and "1m" in only:
        import numpy as np

        n = CONFIG3_CELLS
        Xm = np.empty((n, G), dtype=np.float32)
        for r0 in range(0, n, 50_000):
            Xm[r0:r0 + 50_000] = synth_rows(torch, r0, min(n, r0 + 50_000), G).cpu().numpy()
        torch.cuda.empty_cache()
        _e2e_run(f"dense fp32 {n} x 20000, window 100 (north_star's 1 M cells from host memory, one GPU)", Xm, 100, legs,
                 devices=[0], repeats=2)
        _e2e_run(f"dense fp32 {n} x 20000, window 100, reference=None (1 M cells from host memory, one GPU)", Xm, 100,
                 legs, devices=[0], repeats=2, default_reference=True)
        del Xm
    else:
        legs["dense fp32 1000000 x 20000 from host memory"] = {"skipped": f"needs ~130 GB of free host RAM, {avail / 1e9:.0f} GB available"}
    return legs


def e2e_multi_gpu(torch, devices, cells_per_gpu=100_000):
    """ONE public call over all GPUs of the job (rank 0; the other ranks idle): weak-scaled dense input."""
    import numpy as np

    legs = {}
    try:  # the host copy of the input must fit comfortably (64 GB at 8 x 100 000 cells): a quarter of what is free
        import psutil

        room = psutil.virtual_memory().available // 4
        cells_per_gpu = int(max(5_000, min(cells_per_gpu, room // (G * 4 * len(devices)) // 5_000 * 5_000)))
    except ImportError:
        pass
    n = cells_per_gpu * len(devices)
    Xd = np.empty((n, G), dtype=np.float32)
    for r0 in range(0, n, 50_000):  # generated on this rank's GPU, 4 GB at a time
        r1 = min(n, r0 + 50_000)
        Xd[r0:r1] = synth_rows(torch, r0, r1, G).cpu().numpy()
    torch.cuda.empty_cache()
    _e2e_run(f"dense fp32 {n} x 20000, window 100, tl.infercnv(devices={list(devices)})", Xd, 100, legs,
             devices=list(devices))
    return legs


# ----------------------------------------------------------------------------------------------------------
# HBM-resident step: timing + roofline of the smoothing kernel
# ----------------------------------------------------------------------------------------------------------
def kernel_label(fmt, window, step):
    if fmt == "dense" and window == 100 and step == 10:
        return "k_smooth_x16<10,10,chunk moments> (dense fp32, window 100 / step 10)"
    if fmt == "dense" and window == 250 and step == 10:
        return "k_smooth_x16<5,50,chunk moments> (dense fp32, window 250 / step 10)"
    if fmt == "csr" and window % 2 == 0 and math.gcd(step, window // 2) > 1:
        return ("k_se_table + k_se_wtab + k_smooth_se (CSR fp32, block form: stored entries only, differences to the "
                "zero row in fixed-point block bins, windows from prefix sums)")
    if fmt == "csr":
        return "k_smooth<CSR> (generic: one row in LDS)"
    return "k_smooth_ws (variant for this window; generic k_smooth if the plan does not fit)"


def pmc_traffic(key, cells):
    """HBM bytes per launch from the committed PMC passes (profiles/pmc_traffic.json: FETCH_SIZE / WRITE_SIZE collected
    in separate rocprofv3 --pmc runs on a fixed number of cells, corrected per MI355X_MICROARCH.md), scaled to the
    cells of this launch.  None for workloads without counter data."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        rec = json.load(open(path))
    except Exception:
        return None
    ent = rec.get("kernels", {}).get(key) if "kernels" in rec else None
    if ent is None and key == "dense_w100" and "x16" in rec.get("kernel", ""):
        ent = {"hbm_bytes_per_launch": rec.get("k_smooth_hbm_bytes_per_launch"), "cells": 100_000}
    if not ent or not ent.get("hbm_bytes_per_launch"):
        return None
    return ent["hbm_bytes_per_launch"] * (cells / float(ent.get("cells", 100_000)))


def hbm_step(torch, icd, _engine, plan, dm, n_local, fmt, window, step, chunksize, steps, warmup, dist=None,
             bounds=None, row0=0, n_total=None, no_refmean=False, nnz_row=G, traffic_key=None, pack=False,
             means="allreduce", keep_last=None):
    """Time `steps` passes of the per-rank hot path (dist.run_shard) over the resident rows of `dm`; returns (seconds,
    roofline dict); the last step's return value is appended to the list `keep_last` if one is given.
    means = "blocks": the reference's own bits with the ranks' passes CONCURRENT -- the float32 chain by integer blocks
    (dist.reference_means_blocks: float64 totals, one all-gather, block records, a scan that travels);
    "chained": the reference's own bits -- icv_colchain accumulators handed from rank to rank,
    pipelined over column groups (dist.reference_means_chained), the same computation as the N = 1 public call;
    "allreduce": float64 column sums + ONE all-reduce (correctly rounded means, concurrent)."""
    n_total = n_local if n_total is None else n_total
    W = plan.n_windows
    out = _engine.alloc_out(n_local, W)
    sums = torch.zeros((1, G), dtype=torch.float64, device="cuda")
    fixed_ref = (_engine.column_sums(dm)[0] / n_local).float() if no_refmean else None

    def one_step():
        if fixed_ref is not None:
            ref = fixed_ref
        elif means == "blocks":
            ref = icd.reference_means_blocks(dm, n_total)[0]
        elif means == "chained":
            ref = icd.reference_means_chained(dm, [n_total])[0]
        else:
            sums.zero_()
            _engine.column_sums(dm, None, 1, sums)
            # the only collective of the path: [G] float64 sums + the row count, over RCCL / xGMI
            ref = icd.reference_means(sums, [n_local], "float32", device_out=True)[0] if dist is not None \
                else (sums[0] / n_local).float()
        # no host synchronisation inside a step: the library records HIP events around the smoothing kernel on
        # the launch stream (icv_profile_begin) and the times are read after the timed region
        return icd.run_shard(plan, dm, ref, global_row0=row0, n_obs_global=n_total, lfc_clip=3.0,
                             dynamic_threshold=1.5, chunksize=chunksize, all_bounds=bounds, out=out, pack=pack)

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(warmup):
        one_step()
    fence()
    _engine.profile_begin(plan)
    t0 = time.perf_counter()
    for _ in range(steps):
        last = one_step()
    fence()
    dt = time.perf_counter() - t0
    if keep_last is not None:
        keep_last.append(last)
    smooth_ms = [r.smooth_ms for r in _engine.profile_collect(plan)]
    assert len(smooth_ms) == steps
    # dense 4*G + 4*W = 87 208 B/cell at window 100 / step 10; CSR 8*nnz_row + 8 + 4*W
    bytes_per_cell = (4 * G + 4 * W) if fmt == "dense" else (8 * nnz_row + 8 + 4 * W)
    avg = sum(smooth_ms) / max(len(smooth_ms), 1)
    achieved = bytes_per_cell * n_local / (avg * 1e-3) / 1e9
    roof = {
        "kernel": kernel_label(fmt, window, step), "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
        "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": pmc_traffic(traffic_key, n_local) if traffic_key else None,
        "bytes_per_cell": bytes_per_cell, "kernel_ms": avg, "kernel_ms_min_max": [min(smooth_ms), max(smooth_ms)],
        "cells_per_launch": n_local,
    }
    del out
    return dt, roof


def api_step(torch, _engine, ad, steps, warmup, fmt, window, step, nnz_row=G, traffic_key=None, **kw):
    """Time `steps` calls of cnv.tl.infercnv(ad) on the HBM-resident matrix in ad.X; returns (seconds, roofline of the
    smoothing kernel from the library's own events, X_cnv entry count)."""
    import infercnvpy_amd as cnv
    from infercnvpy_amd.tl import _infercnv as T

    for _ in range(max(warmup, 1)):
        cnv.tl.infercnv(ad, window_size=window, step=step, **kw)
    torch.cuda.synchronize()
    plan = T._cached_plan(ad.var["chromosome"].to_numpy(), ad.var["start"].to_numpy(), window, step,
                          kw.get("exclude_chromosomes", ("chrX", "chrY")), torch.cuda.current_device())
    W, n_local = plan.n_windows, ad.X.shape[0]
    _engine.profile_begin(plan)
    t0 = time.perf_counter()
    for _ in range(steps):
        cnv.tl.infercnv(ad, window_size=window, step=step, **kw)
    t_issued = time.perf_counter() - t0  # host time to ISSUE the steps (the calls are asynchronous); == dt: host bound
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    smooth_ms = [r.smooth_ms for r in _engine.profile_collect(plan)]
    assert len(smooth_ms) == steps, (len(smooth_ms), steps)
    # dense 4*G + 4*W = 87 208 B/cell at window 100 / step 10; CSR 8*nnz_row + 8 + 4*W
    bytes_per_cell = (4 * G + 4 * W) if fmt == "dense" else (8 * nnz_row + 8 + 4 * W)
    avg = sum(smooth_ms) / len(smooth_ms)
    achieved = bytes_per_cell * n_local / (avg * 1e-3) / 1e9
    roof = {
        "kernel": kernel_label(fmt, window, step), "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
        "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": pmc_traffic(traffic_key, n_local) if traffic_key else None,
        "bytes_per_cell": bytes_per_cell, "kernel_ms": avg, "kernel_ms_min_max": [min(smooth_ms), max(smooth_ms)],
        "cells_per_launch": n_local, "host_issue_ms_per_step": t_issued / steps * 1e3,
    }
    return dt, roof, ad.obsm["X_cnv"].nnz()


def _roof(bytes_, ms, extra=None):
    gbs = bytes_ / (ms * 1e-3) / 1e9
    r = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
         "bytes_per_launch": bytes_, "kernel_ms": ms}
    r.update(extra or {})
    return r


def stage_times(torch, _engine, plan, dm, n_local, chunksize, fmt, nnz_row=G, iters=10, mean_traffic=None):
    """The kernels of the public call one by one (engine-level calls as tl.infercnv makes them, events on the launch
    stream): reference-order means, smoothing + chunk thresholds, threshold + CSR pack; each with its roofline.
    Two untimed iterations first (the second one finds the caching allocator warm: every iteration frees its result
    buffers -- 21.6 GB at 1 M cells -- before the next one asks for them, so no timed stage waits for an allocation);
    at least ten timed ones; median (the figure used) and min per stage."""
    W = plan.n_windows
    iters = max(int(iters), 10)
    ms = {"k_colchain": [], "smooth_and_thresholds": [], "threshold_and_csr_pack": []}
    nnz = 0
    is_csr = fmt == "csr"
    for it in range(iters + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        acc = _engine.column_chain(dm, None, None, n_local)
        ref = _engine.chain_mean(acc, n_local, is_csr)
        ev[1].record()
        res = _engine.run_hot_path(plan, dm, ref, chunksize=chunksize, apply=False)
        ev[2].record()
        pk = _engine.threshold_csr(plan, dm, ref, None, res, lfc_clip=3.0, chunksize=chunksize)
        ev[3].record()
        torch.cuda.synchronize()
        if it == 0:
            nnz = pk.nnz()
        if it >= 2:
            for k, (a, b) in zip(ms, ((0, 1), (1, 2), (2, 3))):
                ms[k].append(ev[a].elapsed_time(ev[b]))
        del res, pk, acc, ref
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    in_bytes = (4 * G if not is_csr else 8 * nnz_row + 8) * n_local
    return {
        "kernel_ms": med, "kernel_ms_min": {k: min(v) for k, v in ms.items()}, "iterations": iters,
        "sum_ms": sum(med.values()), "x_cnv_nnz": nnz,
        "roofline_k_colchain": _roof(in_bytes, med["k_colchain"], {
            "traffic": (sum(t for t in (pmc_traffic(k, n_local) for k in mean_traffic) if t) or None) if mean_traffic else None,
            "note": "one pass over the matrix; CSR: + k_csr_tile_bounds16 (column indices once more, 2 B per tile and "
                    "row); traffic: HBM bytes of the stage's kernels from the committed PMC passes (profiles/"
                    "pmc_traffic.json), scaled to the cells of this launch"}),
        "roofline_smooth_and_thresholds": _roof(
            ((4 * G if not is_csr else 8 * nnz_row + 8) + 4 * W) * n_local, med["smooth_and_thresholds"],
            {"note": "the smoothing kernel + the per-chunk threshold kernel; algorithmic bytes as the main roofline"}),
        "roofline_threshold_and_csr_pack": _roof((4 * W + 8) * n_local + 12 * nnz, med["threshold_and_csr_pack"], {
            "kernels": "k_thr_mask_ring (+ k_thr_mask_ties) + k_row_block_sums + k_row_offsets + k_csr_fill_ring",
            "note": "algorithmic bytes: x_res once (4 W per cell) + 12 B per kept entry + 8 B row offset; the mask "
                    "pass and the fill pass each stream x_res through an LDS ring (x_res is read twice, the keep-mask "
                    "-- W / 8 bytes per cell -- written and read once)"}),
    }


def config5_leg(torch, _engine, n=None, d=5000, clusters=30):
    if n is None:  # BASELINE config 5 is 200 000 x 5 000: 240 GB of distances with the Ward rounds' spare columns
        free_b = _engine.free_hbm_bytes()
        n = 200_000 if free_b >= 250e9 else 100_000
    gen = torch.Generator(device="cuda").manual_seed(n)
    centres = torch.randn((clusters, d), device="cuda", generator=gen) * 0.3
    lab = torch.randint(0, clusters, (n,), device="cuda", generator=gen)
    x = centres[lab] + 0.2 * torch.randn((n, d), device="cuda", generator=gen)
    _engine.pairwise_sqeuclidean(x[:256].contiguous())  # warm-up
    d2 = torch.empty((n, (n + (n + 1) // 2 + 3) // 4 * 4), dtype=torch.float32, device="cuda")[:, :n]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    _engine.pairwise_sqeuclidean(x, out=d2)
    e1.record()
    torch.cuda.synchronize()
    t_pd = time.perf_counter() - t0
    t_ev = e0.elapsed_time(e1) * 1e-3  # on the stream: centring (3 small kernels) + k_gram_mfma, no allocation waits
    t0 = time.perf_counter()
    _, rounds = _engine.ward_linkage(d2, spare=True)
    t_w = time.perf_counter() - t0
    tf = 1.0 * n * (n + 128) * d / t_ev / 1e12  # executed flops: tiles on / above the diagonal only
    del d2, x
    torch.cuda.empty_cache()
    return {
        "workload": f"BASELINE config 5 on one GPU{' at half size' if n < 200_000 else ' at full size'}: X_cnv-like "
                    f"{n} x {d} fp32 -> squared Euclidean distances (fp32 MFMA, upper-triangle tiles + mirrored copy) "
                    f"+ Ward linkage",
        "pdist_s": t_pd, "pdist_stream_s": t_ev, "ward_s": t_w, "ward_rounds": rounds,
        "roofline": {"kernel": "k_gram_mfma<DIST,SYM> (stream time of the call: + the three centring / norm kernels, "
                               "< 1 %; the per-kernel split is profiles/r04_config5_rocprofv3_kernel_stats.csv)",
                     "bound": "mfma", "achieved": tf, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": tf / MFMA_F32_PEAK_TFLOPS, "traffic": None},
    }


def _var_frame(cases):
    import pandas as pd

    v = cases.synthetic_var(cases.GENES_PER_CHROM_20K)
    return v, pd.DataFrame({"chromosome": v["chromosome"], "start": v["start"], "end": v["end"]}, index=v["names"])


def extra_legs(torch, icd, _engine, GenePlan, cases, which):
    from infercnvpy_amd._compat import SimpleAnnData
    from infercnvpy_amd.tl import _infercnv as T

    v, var = _var_frame(cases)
    extra = {}

    def leg(name, fn):
        if which and name not in which:
            return
        import gc

        gc.collect()  # what the previous legs left for the cyclic collector is not this leg's time
        t0 = time.perf_counter()
        try:
            extra[name] = fn()
            extra[name]["leg_wall_s"] = round(time.perf_counter() - t0, 2)
        except Exception as e:  # one failing leg must not cost the main line
            extra[name] = {"error": repr(e)}
        torch.cuda.empty_cache()

    def api_leg(ad, cells, fmt, window, label, steps, traffic_key, nnz_row=G):
        dt, roof, nnz = api_step(torch, _engine, ad, steps, 2, fmt, window, 10, nnz_row=nnz_row, traffic_key=traffic_key)
        plan = T._cached_plan(var["chromosome"].to_numpy(), var["start"].to_numpy(), window, 10, ("chrX", "chrY"),
                              torch.cuda.current_device())
        dm = T._resident_matrix(ad.X, torch)
        mt = ("colchain_dense",) if fmt == "dense" else (("colchain_csrq", "csr_tile_bounds16") if traffic_key else None)
        st = stage_times(torch, _engine, plan, dm, cells, CHUNK, fmt, nnz_row=nnz_row, iters=10, mean_traffic=mt)
        return {"workload": label + "; one cnv.tl.infercnv(adata) call per step on the resident matrix, "
                                    "reference = all-cell mean (in the step), X_cnv as device CSR",
                "ms_per_step": dt / steps * 1e3, "cells_per_s": cells / (dt / steps), "steps": steps,
                "nnz_per_cell": nnz_row, "x_cnv_nnz": nnz, "roofline": roof, "stages": st}

    def csr_leg(cells, window, label, traffic_key):
        ip, ix, dv = synth_csr_on_device(torch, cells, G, 0.07, seed=3)
        dm = _engine.DeviceMatrix(indptr=ip, indices=ix, data=dv, shape=(cells, G))
        return api_leg(SimpleAnnData(dm, var=var), cells, "csr", window, label, 5, traffic_key, dv.numel() / cells)

    leg("config4_csr_w250", lambda: csr_leg(
        500_000, 250, "BASELINE config 4: CSR fp32 500000 x 20000, density 0.07, window 250, step 10, HBM resident",
        "csr_w250"))
    leg("csr_w100", lambda: csr_leg(
        200_000, 100, "CSR fp32 200000 x 20000, density 0.07, window 100 (default arguments on 10x-style input), "
                      "HBM resident", "csr_w100"))

    # ---- the three built rows without a timing before round 6: calculate_gene_values=True, ithcna and
    # cnv_score, on config 2's matrix / on the device-resident X_cnv of that call ------------------------------------
    def scores_and_gene_values():
        import infercnvpy_amd as cnv
        import numpy as np
        import pandas as pd

        cells = CONFIG2_CELLS
        X = synth_rows(torch, 0, cells, G)
        obs = pd.DataFrame({"group": np.repeat(np.array(["g0", "g1", "g2", "g3"]), cells // 4)})
        ad = SimpleAnnData(X, var=var, obs=obs)

        def timed(fn, steps, warm=1):
            for _ in range(warm):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        out = {"workload": f"BASELINE config 2's matrix ({cells} x {G} dense fp32, HBM resident, window 100 / step 10): the "
                           "public calls of SURVEY 8 rows a7 / f2 (calculate_gene_values=True), f3 (ithcna) and a10 "
                           "(cnv_score) on the resident matrix / on the device-resident X_cnv (PackedCsr) it returns"}
        plan = T._cached_plan(var["chromosome"].to_numpy(), var["start"].to_numpy(), 100, 10, ("chrX", "chrY"),
                              torch.cuda.current_device())
        W = plan.n_windows
        # (enough steps that the ~0.7 ms of host work in front of the FIRST call's first kernel -- the GPU is idle then -- is
        # not a tenth of the figure: the calls are asynchronous, in steady state the host runs ahead)
        ms_plain = timed(lambda: cnv.tl.infercnv(ad), 30, 2)
        def gv_call():
            ad.layers.clear()  # (the previous call's 16 GB layer goes back to the allocator first: one buffer, reused --
            cnv.tl.infercnv(ad, calculate_gene_values=True)  # a fresh 16 GB hipMalloc costs ~0.4 s on an untouched box)

        ms_gv = timed(gv_call, 15, 2)
        gv = ad.layers["gene_values_cnv"]
        n_nan = int(torch.isnan(gv[:64]).sum().item())
        del gv
        ad.layers.clear()
        gv_bytes = (4 * G + 8 * G + 4 * W) * cells
        out["gene_values"] = {
            "ms_per_call": ms_gv, "plain_call_ms": ms_plain, "ratio_to_plain_call": ms_gv / ms_plain,
            "cells_per_s": cells / (ms_gv * 1e-3), "nan_entries_in_first_64_rows": n_nan,
            "roofline": _roof(gv_bytes, ms_gv, {
                "traffic": (lambda t: sum(t) if all(t) else None)(
                    [pmc_traffic(k, cells) for k in ("colchain_dense", "dense_w100_windows", "thr_mask_ring",
                                                     "csr_fill_ring", "gene_fused")]),
                "traffic_note": "PMC bytes of the call's five large kernels (profiles/pmc_traffic.json): the matrix is read "
                                "twice (means, smoothing), x_res three times written / read, the float64 windows once each way",
                "note": "whole call (means + smoothing + threshold / CSR pack + gene values) against the algorithmic bytes "
                        "4 G in + 4 W x_res out + 8 G gene values out per cell (the float64 cells x genes layer is the "
                        "reference's output type, tl/_infercnv.py:147-149)"})}
        # the same flag on 10x-style CSR input (k_smooth_se also stores its windows): 100 000 cells, density 0.07, window 100
        ip, ix, dv = synth_csr_on_device(torch, cells, G, 0.07, seed=3)
        adc = SimpleAnnData(_engine.DeviceMatrix(indptr=ip, indices=ix, data=dv, shape=(cells, G)), var=var)
        ms_plain_c = timed(lambda: cnv.tl.infercnv(adc), 30, 2)

        def gv_call_csr():
            adc.layers.clear()
            cnv.tl.infercnv(adc, calculate_gene_values=True)

        ms_gv_c = timed(gv_call_csr, 15, 2)
        nnz_row = dv.numel() / cells
        out["gene_values_csr_w100"] = {
            "ms_per_call": ms_gv_c, "plain_call_ms": ms_plain_c, "ratio_to_plain_call": ms_gv_c / ms_plain_c,
            "nnz_per_cell": nnz_row,
            "roofline": _roof((8 * nnz_row + 8 + 4 * W + 8 * G) * cells, ms_gv_c, {
                "note": "whole call on CSR fp32 input (density 0.07, window 100): 8 B per stored entry in + 4 W x_res out + "
                        "8 G gene values out per cell"})}
        del adc, ip, ix, dv
        x_cnv = ad.obsm["X_cnv"]
        nnz = x_cnv.nnz()
        ms_score = timed(lambda: cnv.tl.cnv_score(ad, "group"), 20, 2)
        ad.obs["group_cat"] = ad.obs["group"].astype("category")  # (what tl.leiden writes: the codes are there already)
        ms_score_cat = timed(lambda: cnv.tl.cnv_score(ad, "group_cat"), 20, 2)
        out["cnv_score"] = {
            "ms_per_call": ms_score, "ms_per_call_categorical_groupby": ms_score_cat, "groups": 4, "x_cnv_nnz": nnz,
            "roofline": _roof(8 * nnz + 16 * cells, ms_score, {
                "note": "whole call incl. its host work (labels -> codes, K sums read back): device part = float64 "
                        "values of the stored entries once (8 B each) + row offsets + per-row sums"})}
        ms_ith = timed(lambda: cnv.tl.ithcna(ad, "group"), 3, 1)
        n_g = cells // 4
        flop = 4.0 * n_g * (n_g + 128) * W
        tf = flop / (ms_ith * 1e-3) / 1e12
        out["ithcna"] = {
            "ms_per_call": ms_ith, "groups": 4, "cells_per_group": n_g, "features": W,
            "roofline": {"kernel": "icv_csr_densify + k_row_normalize + k_gram_mfma<CORR> + the IQR selection (k_count_le4 "
                                   "passes over the n x n correlation matrix), whole call",
                         "bound": "mfma", "achieved": tf, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": tf / MFMA_F32_PEAK_TFLOPS, "traffic": None,
                         "note": "executed flops of the upper-triangle tiles: n (n + 128) d per group"}}
        return out

    leg("scores_and_gene_values", scores_and_gene_values)

    # ---- the same step with adata.var in GENOME order ("benchmarks should report both orders"; BASELINE's
    # configs are specified with a random var permutation = the worst case, real annotations are usually GTF-ordered).
    # Both orders take the scatter form of k_smooth_x16: the variant that forms the block sums straight from an ordered
    # row measured 2.2 x slower (profiles/r06_x16_position_ordered_experiment.txt)
    v_pos, _ = cases.position_ordered(v)
    import pandas as _pd

    var_pos = _pd.DataFrame({"chromosome": v_pos["chromosome"], "start": v_pos["start"], "end": v_pos["end"]},
                            index=v_pos["names"])

    def ordered_leg(X, cells, steps, label):
        ad = SimpleAnnData(X, var=var_pos)
        # (five untimed calls: the result buffers of both generations exist before the clock starts -- a first 2 GB
        # allocation on a box whose VRAM has not been touched costs ~0.15 s)
        dt, roof, nnz = api_step(torch, _engine, ad, steps, 5, "dense", 100, 10, traffic_key=None)
        plan = T._cached_plan(var_pos["chromosome"].to_numpy(), var_pos["start"].to_numpy(), 100, 10, ("chrX", "chrY"),
                              torch.cuda.current_device())
        roof["kernel"] = "k_smooth_x16<10,10,chunk moments> (dense fp32, window 100 / step 10, position-ordered columns)"
        return {"workload": label, "var_order": "position", "kernel_id": int(plan.last_kernel()),
                "ms_per_step": dt / steps * 1e3, "cells_per_s": cells / (dt / steps), "steps": steps, "x_cnv_nnz": nnz,
                "roofline": roof}

    leg("config2_position_ordered_var", lambda: ordered_leg(
        synth_rows(torch, 0, CONFIG2_CELLS, G), CONFIG2_CELLS, 200,
        "BASELINE config 2's matrix with adata.var in genome order (chromosomes one after the other, positions "
        "ascending): one cnv.tl.infercnv(adata) call per step, HBM resident, reference = all-cell mean"))

    def one_million():
        X = synth_rows(torch, 0, CONFIG3_CELLS, G)
        leg_ = api_leg(SimpleAnnData(X, var=var), CONFIG3_CELLS, "dense", 100,
                       "BASELINE config 3's matrix on ONE GPU: dense fp32 1000000 x 20000 (80 GB resident), window 100 "
                       "(the size north_star quotes its targets on)", 3, "dense_w100")
        # the N = 1 point of the scaling curve on the code path the N > 1 lines time (dist.run_shard per rank, one
        # rank here): the same 1 M cells, both forms of the reference means
        dm = _engine.DeviceMatrix(dense=X)
        plan = GenePlan(v["chromosome"], v["start"], window_size=100, step=10)
        scale = {"workload": "BASELINE config 3's 1 000 000 cells on ONE rank through the per-rank code path of "
                             "bench.py --gpus N (means -> dist.run_shard(pack=True)); cells/s comparable with the N > 1 "
                             "lines' value (blocks) / value_chained_means / value_allreduce_means.  On ONE rank the block "
                             "form is two passes over the rows where the chain kernel needs one: it pays from 2 ranks on",
                 "n_gpus": 1, "cells": CONFIG3_CELLS, "steps": 3}
        for form in ("blocks", "chained", "allreduce"):
            dt, roof = hbm_step(torch, icd, _engine, plan, dm, CONFIG3_CELLS, "dense", 100, 10, CHUNK, steps=3,
                                warmup=1, traffic_key="dense_w100", pack=True, means=form)
            scale[form] = {"ms_per_step": dt / 3 * 1e3, "value": CONFIG3_CELLS / (dt / 3), "unit": "cells/s",
                           "smooth_kernel_ms": roof["kernel_ms"], "roofline_frac": roof["frac"]}
        plan.close()
        leg_["scale_n1"] = scale
        try:  # the same 1 M cells with position-ordered columns (sustained clocks)
            leg_["position_ordered_var"] = ordered_leg(X, CONFIG3_CELLS, 3, "the same matrix, adata.var in genome order")
        except Exception as e:
            leg_["position_ordered_var"] = {"error": repr(e)}
        return leg_

    leg("config3_cells_on_one_gpu", one_million)

    def in_place():
        X = synth_rows(torch, 0, CONFIG2_CELLS, G)
        dm = _engine.DeviceMatrix(dense=X)
        plan = GenePlan(v["chromosome"], v["start"], window_size=100, step=10)
        dt, roof = hbm_step(torch, icd, _engine, plan, dm, CONFIG2_CELLS, "dense", 100, 10, CHUNK, steps=50, warmup=3,
                            traffic_key="dense_w100")
        plan.close()
        return {"workload": "the round-3 form of the config-2 step (engine-level calls, not the public function): "
                            "float64 column sums (correctly rounded mean, NOT the reference's own float32 order) + "
                            "smoothing + chunk thresholds + IN-PLACE threshold of the dense x_res, no CSR",
                "ms_per_step": dt / 50 * 1e3, "cells_per_s": CONFIG2_CELLS / (dt / 50), "steps": 50, "roofline": roof}

    leg("in_place_threshold_step", in_place)
    leg("config5", lambda: config5_leg(torch, _engine))
    return extra


def _summary(result):
    """Compact digest of the line: headline, roofline fraction, config 4, the e2e rates, the new legs."""
    def g(d, *ks):
        for k in ks:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return d

    def r(x, n=3):
        return round(float(x), n) if isinstance(x, (int, float)) else None

    out = {"value_cells_per_s": r(result.get("value"), 0), "ms_per_step": r(result.get("ms_per_step")),
           "roofline_frac": r(g(result, "roofline", "frac")), "kernel_ms": r(g(result, "roofline", "kernel_ms"))}
    if "value_allreduce_means" in result:
        out["value_allreduce_means"] = r(result["value_allreduce_means"], 0)
        out["value_chained_means"] = r(result.get("value_chained_means"), 0)
        out["value_blocks_means"] = r(result.get("value_blocks_means"), 0)
    ex = result.get("extra") or {}
    c4 = ex.get("config4_csr_w250") or {}
    if "ms_per_step" in c4:
        out["config4_ms_per_step"] = r(c4["ms_per_step"])
        out["config4_k_smooth_se_ms"] = r(g(c4, "roofline", "kernel_ms"))
        out["config4_stage_ms"] = {k: r(v) for k, v in (g(c4, "stages", "kernel_ms") or {}).items()}
    c3 = ex.get("config3_cells_on_one_gpu") or {}
    if "ms_per_step" in c3:
        out["one_million_cells_ms_per_step"] = r(c3["ms_per_step"])
        out["one_million_cells_roofline_frac"] = r(g(c3, "roofline", "frac"))
    sg = ex.get("scores_and_gene_values") or {}
    if "gene_values" in sg:
        out["gene_values_ms"] = r(g(sg, "gene_values", "ms_per_call"))
        out["gene_values_ratio_to_plain"] = r(g(sg, "gene_values", "ratio_to_plain_call"))
        out["gene_values_roofline_frac"] = r(g(sg, "gene_values", "roofline", "frac"))
        out["gene_values_csr_w100_ms"] = r(g(sg, "gene_values_csr_w100", "ms_per_call"))
        out["cnv_score_ms"] = r(g(sg, "cnv_score", "ms_per_call"))
        out["cnv_score_categorical_ms"] = r(g(sg, "cnv_score", "ms_per_call_categorical_groupby"))
        out["ithcna_ms"] = r(g(sg, "ithcna", "ms_per_call"))
    elif "error" in sg:
        out["scores_and_gene_values_error"] = sg["error"][:200]
    po = ex.get("config2_position_ordered_var") or {}
    if "ms_per_step" in po:
        out["position_ordered_ms_per_step"] = r(po["ms_per_step"])
        out["position_ordered_kernel_ms"] = r(g(po, "roofline", "kernel_ms"))
        out["position_ordered_roofline_frac"] = r(g(po, "roofline", "frac"))
    po1 = c3.get("position_ordered_var") or {}
    if "ms_per_step" in po1:
        out["one_million_position_ordered_roofline_frac"] = r(g(po1, "roofline", "frac"))
    c5 = ex.get("config5") or {}
    if "roofline" in c5:
        out["config5_pdist_s"] = r(c5.get("pdist_stream_s"))
        out["config5_mfma_frac"] = r(g(c5, "roofline", "frac"))
        out["config5_ward_s"] = r(c5.get("ward_s"))
    e2e = result.get("e2e") or {}
    if isinstance(e2e, dict):
        rates = {}
        for k, v in e2e.items():
            if isinstance(v, dict) and "cells_per_s" in v:
                rates[k[:70]] = r(v["cells_per_s"], 0)
        if rates:
            out["e2e_cells_per_s"] = rates
    cb = result.get("cpu_baseline") or {}
    if "value" in cb:
        out["cpu_baseline_cells_per_s"] = r(cb["value"], 0)
    return out


# ----------------------------------------------------------------------------------------------------------
# --dump-outputs: what the timed path returned in its last step, to compare two builds output for output
# ----------------------------------------------------------------------------------------------------------
DUMP_ROWS_BYTES = 32 << 20     # dense float64 rows of X_cnv: every row if they fit, else a seeded sample
DUMP_ROW_STATS = 1_000_000     # per-row sums / entry counts: every row up to this many, else a seeded sample


def dump_outputs(out_dir, x_cnv, chr_pos, suffix="", share=1):
    """Write X_cnv of the last timed step to `out_dir` as float64 .npy files (at most 48 MB / `share`):
      x_cnv_rows       dense rows (float64) of the rows in x_cnv_row_index
      x_cnv_row_index  sorted row indices: every row, or a sample drawn with a fixed seed
      x_cnv_row_sum    sum of every row (a fixed-seed sample of DUMP_ROW_STATS rows above that many)
      x_cnv_row_nnz    stored entries of the same rows
      chr_pos          first window of every chromosome, in the plan's chromosome order
    x_cnv: the PackedCsr of the public call / run_shard(pack=True), or the dense device x_res of run_shard(pack=False)
    (whose entries below the threshold are zero, so "stored" = non-zero).  `suffix` tells the files of ranks apart;
    `share` (the number of ranks) divides the budget between them."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    if hasattr(x_cnv, "to_scipy"):
        m = x_cnv.to_scipy()
        n, w = m.shape
        dense_rows = lambda rows: m[rows].toarray()  # noqa: E731
        row_sum = np.asarray(m.sum(axis=1), dtype=np.float64).ravel()
        row_nnz = np.diff(m.indptr).astype(np.float64)
    else:
        a = x_cnv.cpu().numpy()
        n, w = a.shape
        dense_rows = lambda rows: a[rows].astype(np.float64)  # noqa: E731
        row_sum = a.sum(axis=1, dtype=np.float64)
        row_nnz = np.count_nonzero(a, axis=1).astype(np.float64)
    rng = np.random.default_rng(20_000)

    def sample(k):
        return np.arange(n) if k >= n else np.sort(rng.choice(n, k, replace=False))

    rows = sample(max(1, DUMP_ROWS_BYTES // share // (8 * max(w, 1))))
    stat_rows = sample(DUMP_ROW_STATS // share)
    arrays = {
        "x_cnv_rows": dense_rows(rows), "x_cnv_row_index": rows,
        "x_cnv_row_sum": row_sum[stat_rows], "x_cnv_row_nnz": row_nnz[stat_rows],
        "chr_pos": np.array([int(p) for p in chr_pos.values()]),
    }
    if len(stat_rows) < n:
        arrays["x_cnv_row_stats_index"] = stat_rows
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), np.ascontiguousarray(arr, dtype=np.float64))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # default: 300 steps = 1 s of timed GPU work (a 20-step region is 65 ms: too short for an outside sampler to see,
    # and short enough to sit inside the boost window of the clocks)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cells", type=int, default=None, help="total cells (default: 100 000 at N=1, 1 000 000 at N>1)")
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--step", type=int, default=10)
    ap.add_argument("--chunksize", type=int, default=CHUNK)
    ap.add_argument("--format", choices=["dense", "csr"], default="dense",
                    help="csr = BASELINE config 4 style input (not the default bench line)")
    ap.add_argument("--density", type=float, default=0.07)
    ap.add_argument("--full", action="store_true",
                    help="also what takes runs of its own: stages, cpu_baseline, e2e, extra and (N > 1) the all-reduce "
                         "form of the means (a plain run times the headline step only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write X_cnv of the last timed step to DIR as .npy files (a seeded sample; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) without the cpu_baseline leg")
    ap.add_argument("--no-e2e", action="store_true", help="(--full) without the e2e legs")
    ap.add_argument("--no-extra", action="store_true", help="(--full) without the extra legs")
    ap.add_argument("--extra", default="", help="(--full) comma-separated subset of the extra legs (default: all)")
    ap.add_argument("--no-refmean", action="store_true", help="exclude the reference-mean pass from the step")
    ap.add_argument("--engine-step", action="store_true",
                    help="N = 1: time the engine-level step of N > 1 (float64 sums + in-place threshold) instead of "
                         "the public call")
    ap.add_argument("--dry-run-one-gpu", action="store_true",
                    help="NOT a measurement: all ranks on cuda:0, collectives through gloo (prints \"dry_run\": true)")
    args = ap.parse_args()
    if args.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # no launcher: spawn one rank per GPU ourselves (fail loudly rather than report a fake n_gpus)
        import torch

        have = torch.cuda.device_count()
        if have < args.gpus and not args.dry_run_one_gpu:
            sys.exit(f"bench.py: --gpus {args.gpus} requested but this box has {have} visible GPU(s) "
                     f"(--dry-run-one-gpu exercises the N-rank code path on one GPU; it is not a measurement)")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(cmd, env=env))
    world = int(env_world or "1")
    if world != args.gpus:
        sys.exit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}")

    import torch

    import cases
    from infercnvpy_amd import _engine
    from infercnvpy_amd import dist as icd
    from infercnvpy_amd._plan import GenePlan

    quiet_repeated_warnings()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dry = bool(args.dry_run_one_gpu)
    dist = None
    if world > 1:
        import torch.distributed as dist

        if dry:
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            isolated = torch.cuda.device_count() == 1 and any(
                os.environ.get(k) for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"))
            dev_index = 0 if isolated else local_rank  # a launcher may show each rank only its own GPU
            if torch.cuda.device_count() <= dev_index:
                sys.exit(f"bench.py: rank {rank} has no GPU (device_count {torch.cuda.device_count()})")
            torch.cuda.set_device(dev_index)
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        assert dist.get_world_size() == world
    else:
        torch.cuda.set_device(0)
    n_gpus = world

    v = cases.synthetic_var(cases.GENES_PER_CHROM_20K)
    plan = GenePlan(v["chromosome"], v["start"], window_size=args.window, step=args.step)
    W = plan.n_windows
    default_total = CONFIG2_CELLS if n_gpus == 1 else CONFIG3_CELLS
    n_total = args.cells if args.cells is not None else default_total
    if dry and args.cells is None:
        n_total = 20_000 * n_gpus  # small: every rank shares one GPU's HBM
    bounds = icd.shard_bounds(n_total, n_gpus, args.chunksize)
    row0, row1 = bounds[rank]
    n_local = row1 - row0
    if args.format == "dense":
        X = synth_rows(torch, row0, row1, G, chunk=args.chunksize)
        dm = _engine.DeviceMatrix(dense=X)
        nnz_row = G
    else:
        ip, ix, dv = synth_csr_on_device(torch, n_local, G, args.density, seed=3 + rank)
        dm = _engine.DeviceMatrix(indptr=ip, indices=ix, data=dv, shape=(n_local, G))
        nnz_row = dv.numel() / max(n_local, 1)
        X = None
    default_geometry = args.window == 100 and args.step == 10 and args.chunksize == CHUNK
    traffic_key = None
    if args.format == "dense" and default_geometry:
        traffic_key = "dense_w100"
    elif args.format == "csr" and args.step == 10 and args.window in (100, 250) and abs(args.density - 0.07) < 1e-9:
        traffic_key = f"csr_w{args.window}"

    stages = None
    rank_path = n_gpus > 1 or args.engine_step
    if not rank_path:
        # the headline: ONE call of the public function per step on the resident matrix (reference=None: the default)
        from infercnvpy_amd._compat import SimpleAnnData
        from infercnvpy_amd.tl import _infercnv as T

        _, var = _var_frame(cases)
        ad = SimpleAnnData(X if args.format == "dense" else dm, var=var)
        kw = dict(chunksize=args.chunksize)
        if args.no_refmean:
            kw["reference"] = (_engine.column_sums(dm)[0] / n_local).float().cpu().numpy()
        dt, roof, nnz_out = api_step(torch, _engine, ad, args.steps, args.warmup, args.format, args.window, args.step,
                                     nnz_row=nnz_row, traffic_key=traffic_key, **kw)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, ad.obsm["X_cnv"], ad.uns["cnv"]["chr_pos"])
        if args.full:
            api_plan = T._cached_plan(var["chromosome"].to_numpy(), var["start"].to_numpy(), args.window, args.step,
                                      ("chrX", "chrY"), torch.cuda.current_device())
            mt = ("colchain_dense",) if args.format == "dense" else (("colchain_csrq", "csr_tile_bounds16") if traffic_key else None)
            stages = stage_times(torch, _engine, api_plan, dm, n_local, args.chunksize, args.format, nnz_row=nnz_row,
                                 mean_traffic=mt)
            stages["x_cnv_nnz_public_call"] = nnz_out
        ad = None
    else:
        # N > 1 (or --engine-step): the per-rank code path, dist.run_shard, with the thresholds applied while X_cnv is
        # packed to device CSR.  `value` times the CHAINED reference means (the N = 1 public call's own computation:
        # numpy's bits, the ranks pipelined over column groups); the float64 all-reduce form is timed right after it
        # and reported beside it.
        common = dict(dist=dist, bounds=bounds, row0=row0, n_total=n_total, no_refmean=args.no_refmean, nnz_row=nnz_row,
                      traffic_key=traffic_key, pack=not args.engine_step)
        # `value`: the reference's bits.  Dense float32 shards: the chain by integer blocks (the ranks' passes run
        # concurrently); CSR shards: the chained accumulators (the only exact form there)
        first = "blocks" if args.format == "dense" else "chained"
        # (the block form has run under process groups on ONE GPU only: if it fails on every rank of a real multi-GPU job
        # the line still carries the two older forms, and says so)
        first_error = None
        # (the exact forms give the same X_cnv: the dump is that of whichever ran last)
        last = [] if args.dump_outputs else None
        try:
            dt, roof = hbm_step(torch, icd, _engine, plan, dm, n_local, args.format, args.window, args.step,
                                args.chunksize, args.steps, args.warmup, means=first, keep_last=last, **common)
        except Exception as e:  # pragma: no cover
            first_error = repr(e)[:300]
            torch.cuda.synchronize()
        dt_ch, roof_ch = hbm_step(torch, icd, _engine, plan, dm, n_local, args.format, args.window, args.step,
                                  args.chunksize, args.steps, args.warmup, means="chained", keep_last=last, **common)
        if first_error is not None:
            dt, roof = dt_ch, roof_ch
        if last:
            out = last[-1][1] if isinstance(last[-1], tuple) else last[-1].out  # PackedCsr | x_res thresholded in place
            dump_outputs(args.dump_outputs, out, plan.chr_pos, suffix=f".rank{rank}" if world > 1 else "", share=world)
            del last, out
        dt_ar = None
        if args.full:
            dt_ar, roof_ar = hbm_step(torch, icd, _engine, plan, dm, n_local, args.format, args.window, args.step,
                                      args.chunksize, args.steps, args.warmup, means="allreduce", **common)
    if dist is not None:
        t = torch.tensor([dt, dt_ar or 0.0, dt_ch], dtype=torch.float64, device="cpu" if dry else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt, dt_ar, dt_ch = float(t[0].item()), float(t[1].item()) if args.full else None, float(t[2].item())

    def host_barrier(tag):
        """Ranks meet through the rendezvous store (CPU only): no collective kernel spins on the idle GPUs while rank
        0 drives them in the e2e leg, and no second process group (gloo prints to stdout) is created."""
        try:
            store = dist.distributed_c10d._get_default_store()
            store.set(f"icv_bench_{tag}_{rank}", b"1")
            store.wait([f"icv_bench_{tag}_{r}" for r in range(world)])
        except Exception:
            dist.barrier()


    # N > 1, dense shards: two exact forms of the means were timed (same bits): `value` is the faster one at this rank
    # count -- the blocks pay two concurrent passes + a scan (~2.2 passes of a rank's rows), the chained accumulators
    # (T + R - 1) / T passes with T = 2: 1.5 at R = 2, 2.5 at R = 4, 4.5 at R = 8 (dist.reference_means_exact picks alike)
    value_form, dt_blocks = None, None
    if rank_path and dist is not None and args.format == "dense" and not args.engine_step:
        if first_error is None:
            dt_blocks = dt
            value_form = "blocks"
            if dt_ch < dt:
                dt, roof, value_form = dt_ch, roof_ch, "chained"
        else:
            value_form = "chained"
    ms_per_step = dt / args.steps * 1e3
    value = n_total / (dt / args.steps)

    if args.format == "dense" and default_geometry and n_total == default_total:
        name = "BASELINE config 2: dense fp32" if n_gpus == 1 else "BASELINE config 3: dense fp32"
    elif args.format == "csr" and args.window == 250 and args.step == 10 and n_total == 500_000 and n_gpus == 1:
        name = f"BASELINE config 4: CSR fp32 density {args.density}"
    else:
        name = ("custom (not a BASELINE configuration): " +
                ("dense fp32" if args.format == "dense" else f"CSR fp32 density {args.density}"))
    result = {
        "metric": (f"cells/sec through tl.infercnv (window={args.window}), input resident in HBM" if not rank_path else
                   f"cells/sec through the tl.infercnv hot path (window={args.window}) as dist.run_shard on every rank "
                   f"(reference-order means: the faster of the chain by integer blocks and the chained accumulators, "
                   f"see forms), input resident in HBM"),
        "value": value,
        "unit": "cells/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        # total work per N is fixed for N > 1 (config 3: 1 M cells); N = 1 runs config 2 (100 000 cells) as BASELINE
        # asks, and the same 1 M cells on one GPU are the `extra.config3_cells_on_one_gpu` leg of the N = 1 line.
        # The step is linear in cells, so cells/s are comparable across all N.
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",  # arithmetic type from the block sums on (np.convolve is float64); I/O is float32
        "data": "synthetic",
        "config": {
            "workload": f"{name} {n_total} cells x {G} genes (chr1..22, random var order), "
                        f"window {args.window}, step {args.step}, chunksize {args.chunksize}, lfc_clip 3, "
                        f"dynamic_threshold 1.5, reference = all-cell mean"
                        + (" (precomputed, excluded from the step)" if args.no_refmean else " (in the step)")
                        + ("; step = one cnv.tl.infercnv(adata) call, adata.X a CUDA tensor, X_cnv returned as device "
                           "CSR float64 (reference-order means, smoothing, noise threshold + CSR pack)"
                           if not rank_path else
                           "; step = reference-order column means (numpy's own bits: the float32 chain by integer "
                           "blocks, dist.reference_means_blocks -- float64 totals + one all-gather + block records on "
                           "every rank at once, then a scan over the records from rank to rank) + smoothing + thresholds "
                           + ("applied while X_cnv is packed to device CSR (dist.run_shard(pack=True))" if not args.engine_step
                              else "applied in place (dist.run_shard)")),
            "io_dtype": "f32 matrix in, f32 x_res out",
            "var_order": "random (BASELINE's worst case; extra.config2_position_ordered_var has the genome order)",
            "cells_total": n_total,
            "cells_per_gpu": [b - a for a, b in bounds],
            "n_windows": W,
            "scaling_note": "N = 1: BASELINE config 2 (100 000 cells); N > 1: config 3 (1 000 000 cells in total, "
                            "sharded): fixed total work for N > 1",
            "parallelism": f"{n_gpus} rank(s) (torch.distributed world size "
                           f"{dist.get_world_size() if dist is not None else 1}, backend "
                           f"{('gloo, ALL RANKS ON cuda:0 (dry run)' if dry else 'nccl/RCCL') if dist is not None else 'none'}), "
                           + ("row shards aligned to the chunks; value: one all-gather of [G] float64 totals, the [G] float32 "
                              "chain values travel rank to rank point to point in 4 column groups behind a scan of the "
                              "block records, one broadcast of the means; value_chained_means: the accumulators of the "
                              "chain kernel travel instead (the ranks' passes take turns); value_allreduce_means: "
                              "one all-reduce of the [G+1] float64 reference sums per step; no other collective"
                              if n_gpus > 1 else "one GPU, no collective"),
        },
        "roofline": roof,
    }
    if rank_path:
        if dt_ar is not None:
            result["value_allreduce_means"] = n_total / (dt_ar / args.steps)
            result["ms_per_step_allreduce_means"] = dt_ar / args.steps * 1e3
        result["value_chained_means"] = n_total / (dt_ch / args.steps)
        result["ms_per_step_chained_means"] = dt_ch / args.steps * 1e3
        if dt_blocks is not None:
            result["value_blocks_means"] = n_total / (dt_blocks / args.steps)
            result["ms_per_step_blocks_means"] = dt_blocks / args.steps * 1e3
        result["forms"] = {
            "value": ("reference means in the reference's own evaluation order, X_cnv bit-identical to the one-GPU public "
                      "call for any number of ranks; the FASTER of the two exact forms at this rank count (both timed: "
                      "value_blocks_means, value_chained_means) = " +
                      ("value_blocks_means: the float32 chain by integer blocks WITHOUT the ranks taking turns "
                       "(dist.reference_means_blocks: every rank adds float64 totals and forms its block records "
                       "concurrently, one all-gather, a scan over the records travels rank to rank)"
                       if value_form == "blocks" else
                       "value_chained_means (the chain by integer blocks -- value_blocks_means -- pays two passes over a "
                       "rank's rows and wins from ~4 ranks on)")
                      if args.format == "dense" else
                      "CSR shards: the chained accumulators (value = value_chained_means)"),
            "value_blocks_means": "the float32 chain by integer blocks (dist.reference_means_blocks), dense shards",
            "value_chained_means": "the same bits with the icv_colchain accumulators handed from rank to rank, pipelined "
                                   "over 2 column groups (dist.reference_means_chained; rounds 4-5: the ranks take turns)",
        }
        if dt_ar is not None:
            result["forms"]["value_allreduce_means"] = (
                "float64 column sums + one all-reduce (dist.reference_means): correctly rounded means, concurrent over "
                "the ranks, ~1e-3 of the X_cnv entries next to the noise threshold may differ from the reference "
                "(tl.infercnv(mean_order='float64'))")
            result["forms"]["smooth_kernel_ms_allreduce_run"] = roof_ar["kernel_ms"]
        if first_error is not None:
            result["forms"]["value"] = "THE BLOCK FORM FAILED (" + first_error + "): value = value_chained_means"
    if stages is not None:
        result["stages"] = stages
    if dry:
        result["dry_run"] = True
        result["dry_run_note"] = ("all ranks share ONE GPU and the collectives go through gloo and the host: code-path "
                                  "exercise only, the numbers mean nothing")
    del X, dm
    torch.cuda.empty_cache()
    if args.full and rank == 0 and n_gpus == 1 and args.format == "dense":
        if not args.no_cpu_baseline:
            try:
                result["cpu_baseline"] = cpu_baseline(window=args.window, step=args.step)
            except Exception as e:  # the GPU number must still be reported
                result["cpu_baseline"] = {"error": repr(e)}
        if not args.no_e2e:
            try:
                result["e2e"] = e2e_legs(torch)
            except Exception as e:
                result["e2e"] = {"error": repr(e)}
        if not args.no_extra and default_geometry and args.cells is None:
            which = [w for w in args.extra.split(",") if w]
            result["extra"] = extra_legs(torch, icd, _engine, GenePlan, cases, which)
            leg3 = result["extra"].get("config3_cells_on_one_gpu")
            if isinstance(leg3, dict) and "scale_n1" in leg3:
                result["scale_n1"] = leg3.pop("scale_n1")
    if args.full and n_gpus > 1 and not args.no_e2e and args.format == "dense":
        # the public API over all GPUs of the job, from host memory: rank 0 drives every GPU from one process while
        # the other ranks have released their HBM and wait
        torch.cuda.synchronize()
        host_barrier("e2e_begin")
        if rank == 0:
            try:
                # (a launcher that shows each rank only its own GPU leaves rank 0 one device: the leg then says so)
                devs = [0] * n_gpus if dry else list(range(min(n_gpus, torch.cuda.device_count())))
                result["e2e"] = e2e_multi_gpu(torch, devs, cells_per_gpu=10_000 if dry else 100_000)
            except Exception as e:
                result["e2e"] = {"error": repr(e)}
        host_barrier("e2e_end")
    if rank == 0:
        # the figures a reader of a TRUNCATED record needs, as the LAST key of the line (a driver keeps the tail of the
        # output) and once more as a short line of its own before it; the ONE JSON line is the last line printed
        result["summary"] = _summary(result)
        sys.stdout.flush()
        print("bench-summary " + json.dumps(result["summary"]), file=sys.stderr, flush=True)
        print(json.dumps(result), flush=True)
    if dist is not None:
        host_barrier("exit")
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

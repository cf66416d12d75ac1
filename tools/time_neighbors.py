"""Stage split of pp.neighbors on PCA-like points (Gaussian mixture, anisotropic spread, 50 float32 columns,
HBM-resident), plus a host baseline (sklearn brute force + the numpy oracle's fuzzy step).

    python tools/time_neighbors.py [--cells 100000 1000000] [--k 15] [--runs 3] [--host-cells 20000]

Stages: centring, candidate sweep, re-rank and exact fallback are the device times icv_knn reports (HIP events around
its own launches); fuzzy (icv_knn_fuzzy), symmetrise (count + offsets + fill + sort, and the distances' row sort) and
copy-back are wall times with the GPU synchronised after each; total is one pp.neighbors call from a CUDA tensor.
The sweep's rate counts the arithmetic it executes, n_pad^2 * 2 * d_padded flop, against the 155 TFLOP/s the fp32 MFMA
sequence sustains (tools/bench_gram.hip)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MFMA_TFLOPS = 155.0


def points(n, d=50, seed=0, n_clusters=8):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = 3.0 / torch.sqrt(torch.arange(d, device="cuda") + 1.0)
    centres = torch.randn((n_clusters, d), generator=g, device="cuda") * scale * 2.0
    lab = torch.randint(0, n_clusters, (n,), generator=g, device="cuda")
    return (centres[lab] + torch.randn((n, d), generator=g, device="cuda") * scale).float().contiguous()


def stage_split(n, k, d=50):
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine
    from infercnvpy_amd._compat import SimpleAnnData

    x = points(n, d)
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return time.perf_counter() - t0, out

    ms = []
    t_knn, (idx, dist, n_exact) = timed(lambda: _engine.knn(x, k, stage_ms=ms))
    t_fuzzy, (rho, sigma, w) = timed(lambda: _engine.knn_fuzzy(dist, k))
    t_sym, (c, dm) = timed(lambda: (_engine.knn_symmetrize(idx, w, k), _engine.knn_sorted_rows(idx, dist)))
    t_copy, _ = timed(lambda: [t.cpu() for t in (*c, *dm)])
    ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obsm={"X_cnv_pca": x})
    t_total, _ = timed(lambda: cnv.pp.neighbors(ad, n_neighbors=k))
    dp = 64 if d <= 64 else 128 if d <= 128 else 256
    n_pad = -(-n // 128) * 128
    tflops = 2.0 * n_pad * n_pad * dp / (ms[1] * 1e-3) / 1e12
    return dict(cells=n, d=d, k=k, centre_s=ms[0] * 1e-3, sweep_s=ms[1] * 1e-3, rerank_s=ms[2] * 1e-3,
                exact_fallback_s=ms[3] * 1e-3, rows_exact=n_exact, knn_wall_s=t_knn, fuzzy_s=t_fuzzy,
                symmetrise_s=t_sym, copy_back_s=t_copy, total_s=t_total, sweep_tflops=tflops,
                sweep_fraction_of_mfma_rate=tflops / MFMA_TFLOPS)


def host_baseline(n, k, d=50):
    from sklearn.neighbors import NearestNeighbors

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import _neighbors_oracle as O

    x = O.mixture(n, d, seed=0)
    t0 = time.perf_counter()
    dist, idx = NearestNeighbors(n_neighbors=k, algorithm="brute", n_jobs=16).fit(x).kneighbors(x)
    t1 = time.perf_counter()
    _, _, w, _ = O.smooth(dist[:, 1:].astype(np.float32), k)
    O.connectivities_csr(idx[:, 1:].astype(np.int32), w)
    t2 = time.perf_counter()
    return dict(cells=n, d=d, k=k, sklearn_brute_s=t1 - t0, numpy_fuzzy_s=t2 - t1, host_total_s=t2 - t0,
                cpus=len(os.sched_getaffinity(0)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-cells", type=int, default=20000)
    a = ap.parse_args()
    for n in a.cells:
        for run in range(a.runs):
            print(json.dumps(dict(run=run, **stage_split(n, a.k))), flush=True)
    if a.host_cells:
        print(json.dumps(dict(run=0, **stage_split(a.host_cells, a.k))), flush=True)
        print(json.dumps(host_baseline(a.host_cells, a.k)), flush=True)

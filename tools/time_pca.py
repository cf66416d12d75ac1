"""Stage split of tl.pca on an X_cnv-like matrix at the 20 000-gene geometry (1 802 windows, 13 % stored entries,
float32 values widened to float64, HBM-resident as tl.infercnv leaves it), plus a host sklearn baseline.

    python tools/time_pca.py [--cells 100000 1000000] [--sklearn-cells 20000] [--mfma-tflops X]

Stages (wall time, GPU synchronised after each): densify (icv_csr_densify of the same rows: the panel fill inside
icv_gram_f64 does this work), Gram (icv_gram_f64 including its panel fill), copy-back of G, host eigh, projection
(icv_project, X_pca to the host), total (one tl.pca call).  Gram TFLOP/s counts the n * W^2 flops of the full
product as the task is usually quoted and the n * W (W + 1) / 2 * 2 executed on the triangle."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_packed(n, w, density, seed=0):
    import torch

    from infercnvpy_amd import PackedCsr

    g = torch.Generator(device="cuda").manual_seed(seed)
    ind, val, cnt = [], [], []
    for r0 in range(0, n, 65536):
        r1 = min(n, r0 + 65536)
        mask = torch.rand((r1 - r0, w), generator=g, device="cuda") < density
        cnt.append(mask.sum(1))
        ind.append(mask.nonzero()[:, 1].to(torch.int32))
        val.append((torch.randn(int(ind[-1].numel()), generator=g, device="cuda") * 0.1).double())
        del mask
    counts = torch.cat(cnt)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(counts, 0, out=indptr[1:])
    return PackedCsr(indptr, torch.cat(ind), torch.cat(val), w)


def stage_split(n, w=1802, density=0.13, k=50):
    import scipy.linalg
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine
    from infercnvpy_amd._compat import SimpleAnnData

    x = synthetic_packed(n, w, density)
    sync = torch.cuda.synchronize

    def timed(fn, reps=3):
        best, out = 1e30, None
        for _ in range(reps):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            best = min(best, time.perf_counter() - t0)
        return best, out

    t_dens, _ = timed(lambda: x.dense_rows())
    torch.cuda.empty_cache()
    inp = _engine._PcaInput(x)
    t_gram_copy, (g, s) = timed(lambda: _engine.gram(inp, zero_center=True))
    gd = torch.from_numpy(g).cuda()
    t_copy, _ = timed(lambda: gd.cpu())
    t_eigh, (lam, v) = timed(lambda: scipy.linalg.eigh(g, subset_by_index=[w - k, w - 1], driver="evr"))
    t_proj, _ = timed(lambda: _engine.project(inp, np.ascontiguousarray(v[:, ::-1]), None, np.float32))
    ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    t_total, _ = timed(lambda: cnv.tl.pca(ad), reps=2)
    t_gram = t_gram_copy - t_copy
    flops_full = 2.0 * n * w * w
    flops_tri = 2.0 * n * w * (w + 1) / 2
    return dict(cells=n, windows=w, nnz=int(x.nnz()), densify_s=t_dens, gram_s=t_gram, copy_back_s=t_copy,
                eigh_s=t_eigh, projection_s=t_proj, total_s=t_total, gram_tflops_full=flops_full / t_gram / 1e12,
                gram_tflops_executed=flops_tri / t_gram / 1e12)


def sklearn_baseline(n, w=1802, density=0.13):
    import scipy.sparse as sp
    from sklearn.decomposition import TruncatedSVD

    rng = np.random.RandomState(0)
    x = sp.random(n, w, density=density, format="csr", random_state=rng, dtype=np.float64)
    x.data = (rng.standard_normal(x.nnz) * 0.1).astype(np.float32).astype(np.float64)
    t0 = time.perf_counter()
    TruncatedSVD(n_components=50, algorithm="arpack", random_state=0).fit_transform(x)
    return dict(cells=n, windows=w, sklearn_arpack_s=time.perf_counter() - t0, cpus=len(os.sched_getaffinity(0)),
                omp_num_threads=os.environ.get("OMP_NUM_THREADS"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--sklearn-cells", type=int, default=20000)
    ap.add_argument("--mfma-tflops", type=float, default=None, help="measured f64 MFMA rate (tools/bench_mfma_f64.hip)")
    a = ap.parse_args()
    for n in a.cells:
        r = stage_split(n)
        if a.mfma_tflops:
            r["gram_fraction_of_mfma_rate"] = r["gram_tflops_executed"] / a.mfma_tflops
        print(json.dumps(r), flush=True)
    if a.sklearn_cells:
        try:
            print(json.dumps(sklearn_baseline(a.sklearn_cells)), flush=True)
        except ImportError as e:
            print(json.dumps({"sklearn_baseline": f"skipped: {e}"}), flush=True)

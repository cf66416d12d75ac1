"""Stage split of pp.neighbors -> tl.leiden, HBM-resident.

    python tools/time_leiden.py [--sizes 20000,100000,1000000] [--out profiles/leiden_stage_split.txt] [--louvain | --louvain-only]

Mixtures of n cells x 50 components, n_neighbors = 15; one warm-up and three timed runs per size.  A run with
``stages`` synchronises after every phase of every level (events), so the wall time of a plain run is printed
separately.  --louvain also times networkx's Louvain at 20 000 cells on the host: NOT leidenalg (which is not
installed), only what a user of this image had before.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def louvain_line():
    """networkx's Louvain on the host at 20 000 cells x 50 components (needs no GPU)."""
    import networkx as nx

    import _neighbors_oracle as no

    g = no.neighbors(no.mixture(20000, 50, 0), 15)["connectivities"]
    G = nx.from_scipy_sparse_array(g.astype(np.float64), edge_attribute="weight")
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(G, weight="weight", resolution=1.0, seed=0)
    dt = time.perf_counter() - t0
    q = nx.community.modularity(G, parts, weight="weight")
    return (f"networkx louvain_communities (host, NOT leidenalg) n=20000: {dt * 1e3:.0f} ms, {len(parts)} communities, "
            f"Q={q:.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leiden_stage_split.txt"))
    ap.add_argument("--louvain", action="store_true")
    ap.add_argument("--louvain-only", action="store_true", help="append only the host Louvain line to --out")
    args = ap.parse_args()
    if args.louvain_only:
        line = louvain_line()
        print(line)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        return
    import torch

    import _neighbors_oracle as no
    from infercnvpy_amd import _engine

    lines = ["# tools/time_leiden.py: mixture n x 50, n_neighbors = 15, resolution = 1, random_state = 0, n_iterations = -1",
             "# ms; median of 3 runs after a warm-up; staged runs synchronise after every phase (their sum > plain wall)"]
    for n in [int(s) for s in args.sizes.split(",")]:
        x = torch.from_numpy(no.mixture(n, 50, 0)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx, dist, _ = _engine.knn(x, 15)
        _, _, w = _engine.knn_fuzzy(dist, 15)
        indptr, indices, data = _engine.knn_symmetrize(idx, w, 15)
        torch.cuda.synchronize()
        nb_ms = (time.perf_counter() - t0) * 1e3
        nnz = indices.numel()
        walls, staged = [], []
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels, info = _engine.leiden(indptr, indices, data)
            host = labels.cpu()
            torch.cuda.synchronize()
            if rep:
                walls.append((time.perf_counter() - t0) * 1e3)
        for rep in range(3):
            st = []
            _engine.leiden(indptr, indices, data, stages=st)
            staged.append(st)
        med = sorted(walls)[1]
        st = staged[1]
        lines.append(f"n={n} nnz={nnz} neighbors(first call)={nb_ms:.1f} leiden_wall={med:.1f} (runs {', '.join(f'{v:.1f}' for v in walls)}) "
                     f"communities={info['n_communities']} iterations={info['n_iterations']} Q={info['quality'][-1]:.6f} "
                     f"bound_reached={info['bound_reached']} workspace_MB={info['workspace_bytes'] / 1e6:.1f}")
        lines.append(f"  quantise={st[0]['quantise_ms']:.2f}")
        for it, s in enumerate(st):
            lines.append(f"  iteration {it}: local_moving={s['local_moving_ms']:.2f} refinement={s['refinement_ms']:.2f} "
                         f"aggregation={s['aggregation_ms']:.2f} rest={s['rest_ms']:.2f}  levels={info['levels'][it]} "
                         f"rounds(move, refine)={info['rounds'][it]}")
        # level 0, one round of local moving must read: row pointers 8 n, indices 4 nnz, weights 8 nnz, the community
        # of every entry 4 nnz, K_c 8 per candidate (<= 8 nnz), k / comm / want / sel per vertex ~ 28 n
        r0 = info["rounds"][0][0][0]
        bytes_round = 8 * n + (4 + 8 + 4 + 8) * nnz + 28 * n
        lines.append(f"  level 0 local moving: {r0} rounds, >= {bytes_round / 1e6:.1f} MB to read per round")
        del x, idx, dist, w, indptr, indices, data
    if args.louvain:
        lines.append(louvain_line())
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""Record networkx's Louvain modularity on the mixture graphs (the yardstick of the Leiden quality test).

    python tests/golden/make_leiden_golden.py

For n in (2000, 5000) and resolution in (0.5, 1, 2): Q of louvain_communities(seed = 0 .. 9) on pp.neighbors'
connectivities (numpy oracle) of _neighbors_oracle.mixture(n, 10, 0), n_neighbors = 15, evaluated by
networkx.community.modularity on the float64 graph.  Written to tests/golden/leiden/louvain_q.npz as q_<n>_<gamma> (a directory of its own: every *.npz directly under
tests/golden is read as an infercnv case by tests/_golden.py).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SIZES = (2000, 5000)
GAMMAS = (0.5, 1.0, 2.0)
SEEDS = tuple(range(10))


def nx_graph(graph):
    import networkx as nx

    return nx.from_scipy_sparse_array(graph.astype(np.float64).tocsr(), edge_attribute="weight")


def louvain_q(G, gamma, seed):
    import networkx as nx

    parts = nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=seed)
    return nx.community.modularity(G, parts, weight="weight", resolution=gamma)


def labels_q(G, labels, gamma):
    import networkx as nx

    labels = np.asarray(labels)
    parts = [set(np.flatnonzero(labels == c).tolist()) for c in range(int(labels.max()) + 1)]
    return nx.community.modularity(G, parts, weight="weight", resolution=gamma)


def key(n, gamma):
    return f"q_{n}_{gamma}"


if __name__ == "__main__":
    import _leiden_oracle as lo

    out = {}
    for n in SIZES:
        G = nx_graph(lo.mixture_graph(n, 0))
        for gamma in GAMMAS:
            out[key(n, gamma)] = np.array([louvain_q(G, gamma, s) for s in SEEDS])
            print(key(n, gamma), out[key(n, gamma)].min(), out[key(n, gamma)].max(), flush=True)
    os.makedirs(os.path.join(HERE, "leiden"), exist_ok=True)
    np.savez(os.path.join(HERE, "leiden", "louvain_q.npz"), **out)

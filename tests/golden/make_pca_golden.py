#!/usr/bin/env python
"""Record the tl.pca fixtures (tests/golden/pca/pca_*.npz) with sklearn (container-only tool).

    python tests/golden/make_pca_golden.py

The inputs are the X_cnv outputs (``out``) of existing golden cases.  zero_center=False is
``TruncatedSVD(algorithm="arpack")``, zero_center=True is ``PCA(svd_solver="arpack")``, both as scanpy calls them
(n_comps: scanpy's default).  Stored: X_pca in float32 (a row sample for tall cases), the components (a column
sample for wide cases), singular values, explained variance and its ratio.  Data only; the GPU tests read them with
numpy alone.
"""
from __future__ import annotations

import os

import numpy as np
import scipy.sparse as sp
import sklearn
from sklearn.decomposition import PCA, TruncatedSVD

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pca")
CASES = ("big20k_w100_s10", "big20k_w250_s10_csr", "m_densef_f32_9000", "w100_s10_csr_x", "m_w50_s10")


def record(name, zero_center):
    x = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)["out"]
    n, w = x.shape
    k = min(50, min(n, w) - 1)
    X = sp.csr_matrix(x)
    if zero_center:
        est = PCA(n_components=k, svd_solver="arpack", random_state=0)
        x_pca = est.fit_transform(x)
    else:
        est = TruncatedSVD(n_components=k, algorithm="arpack", random_state=0)
        x_pca = est.fit_transform(X)
    rows = np.arange(n) if n <= 1000 else np.arange(0, n, 9)
    cols = np.arange(w) if w <= 200 else np.unique(np.r_[np.arange(0, w, 16), np.argmax(np.abs(est.components_), 1)])
    tag = "pca" if zero_center else "tsvd"
    np.savez_compressed(
        os.path.join(OUT, f"pca_{tag}_{name}.npz"),
        source=name, zero_center=bool(zero_center), n_comps=k, sklearn_version=sklearn.__version__,
        rows=rows, x_pca=x_pca.astype(np.float32)[rows], cols=cols, components=est.components_[:, cols],
        singular_values=est.singular_values_, explained_variance=est.explained_variance_,
        explained_variance_ratio=est.explained_variance_ratio_,
    )


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for name in CASES:
        for zc in (False, True):
            record(name, zc)
    print("\n".join(f"{f} {os.path.getsize(os.path.join(OUT, f))}" for f in sorted(os.listdir(OUT))))

"""Random Ward-linkage / score cases against scipy and numpy (GPU box; test infrastructure like the rest of tests/: it checks the product against oracle/):
    python tests/fuzz_gpu_ward.py [first_seed] [n_seeds]
Per seed: n in 2..1500 cells, d in 4..99 features, 1..10 blobs (now and then with duplicated cells, or without any
structure), both column layouts of the Ward rounds (spare columns / in place).  Checked against scipy's float64
`linkage(method="ward")`: a valid linkage, the multiset of cluster sizes, sorted heights to 2e-4 relative (float32
distances; duplicated cells: 1e-3 of the tallest merge), >= 97 % of the merged leaf sets (merges whose heights agree to
rounding may permute).  And against the numpy oracle of the rounds (tests/_ward_oracle.py) on the GPU's own distance
matrix: the linkage matrix and the round count must be equal, bit for bit.  Then `cnv_score`
and `ithcna` on the same matrix against their numpy restatements."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, _p)


def one_case(seed):
    import numpy as np
    import pandas as pd
    import scipy.sparse as sp
    from scipy.cluster.hierarchy import is_valid_linkage

    import torch

    import infercnvpy_amd as cnv
    import test_gpu_parity as T
    from _ward_oracle import ward_rounds
    from infercnvpy_amd import _engine
    from infercnvpy_amd._compat import SimpleAnnData
    from oracle import infercnv_oracle as O

    rng = np.random.RandomState(70_000 + seed)
    n = int(rng.choice([2, 3, 5, 17, 64, 65, 200, 513, 1000, 1500])) if rng.rand() < 0.5 else int(rng.randint(2, 1500))
    # (d >= 4: in one or two dimensions a cloud of 1 000 points has neighbours ~1e-3 of the cloud's size apart, where the
    # absolute float32 error of the Gram form, ~2e-7 |x||y| on a squared distance, reorders the bottom of the tree --
    # seeds with d = 1, 2 differed from scipy there; X_cnv has thousands of columns)
    d = int(rng.randint(4, 100))
    k = int(rng.randint(1, 11))
    X = T._blobs(n, d, k, seed=seed, spread=float(rng.choice([0.0, 1.0, 4.0])))
    dup = bool(rng.rand() < 0.3 and n > 4)
    if dup:
        m = rng.randint(2, min(n, 12))
        X[:m] = X[0]  # duplicated cells: zero distances
    desc = f"n={n} d={d} k={k} dup={dup}"
    os.environ.pop("ICV_WARD_IN_PLACE", None)
    if seed % 2:
        os.environ["ICV_WARD_IN_PLACE"] = "1"
    T._knobs()  # (the library reads its developer knobs once)
    try:
        Z, rounds = cnv.tl.ward_linkage(X, return_rounds=True)
        d2 = _engine.pairwise_sqeuclidean(torch.from_numpy(X).cuda()).cpu().numpy()
    finally:
        os.environ.pop("ICV_WARD_IN_PLACE", None)
        T._knobs()
    Ze, rounds_e = ward_rounds(d2)  # the rounds alone: an equality, whatever the Gram rounded
    assert rounds == rounds_e, desc + f" rounds {rounds} vs oracle {rounds_e}"
    np.testing.assert_array_equal(Z, Ze, err_msg=desc)
    Zs = O.ward_linkage(X)
    assert Z.shape == Zs.shape == (n - 1, 4), desc
    assert is_valid_linkage(Z), desc
    # cluster sizes: the same multiset unless two candidate merges that share a cluster tie to float32 rounding (then
    # the trees differ locally: heights and >= 97 % of the leaf sets below still have to agree); duplicated cells merge
    # at height 0 in any order in scipy, at rounding-noise heights here
    same_sizes = np.array_equal(np.sort(Z[:, 3]), np.sort(Zs[:, 3]))
    # float32 distances in Gram form: the squared distance of two cells carries an absolute error of ~2e-7 |x||y|, so
    # a pair of DUPLICATED cells merges at ~4e-4 of a typical distance instead of 0; everything else to 2e-4 relative
    scale = max(float(Zs[:, 2].max()), 1e-30)
    hs, hz = np.sort(Z[:, 2]), np.sort(Zs[:, 2])
    tol = 2e-4 * hz + (1e-3 if dup else 1e-6) * scale
    frac_ok = float(np.mean(np.abs(hs - hz) <= tol))
    if same_sizes:
        assert frac_ok == 1.0, desc + f" heights: worst {np.max(np.abs(hs - hz) / tol):.2f} x tolerance, scale {scale}"
    else:
        # a different tree (~0.3 % of the cases): scipy's own tree changes in these very seeds when its squared
        # distances get the float32 Gram-form noise (2e-7 |x||y|) -- checked on the CPU for the first ones found --
        # so only the bulk is compared
        assert frac_ok >= 0.5, desc + f" heights: only {frac_ok:.2f} within tolerance"
    if n > 2:
        mine, ref = T._cluster_hashes(Z), T._cluster_hashes(Zs)
        need = (0.97 if same_sizes else 0.75) * (n - 1) - 2
        assert len(mine & ref) >= need, desc + f" leaf sets {len(mine & ref)} of {n - 1}"
    # scores on the same matrix as X_cnv
    groups = rng.choice(["g0", "g1", "g2"], size=n)
    ad = SimpleAnnData(np.zeros((n, 1), np.float32), obs=pd.DataFrame({"grp": groups}))
    ad.obsm["X_cnv"] = sp.csr_matrix(X.astype(np.float64)) if seed % 3 else X.astype(np.float64)
    got = cnv.tl.cnv_score(ad, groupby="grp", inplace=False)
    for g in np.unique(groups):
        exp = np.mean(np.abs(X[groups == g].astype(np.float64)))
        assert abs(got[g] - exp) <= 1e-9 * max(1.0, abs(exp)), desc + f" cnv_score {g}: {got[g]} vs {exp}"
    # ithcna: IQR of the cell-cell Pearson correlations per group (float32 MFMA Gram matrix vs np.corrcoef: 1e-5)
    if n >= 4:
        g2 = np.where(np.arange(n) % 2 == 0, "even", "odd")
        ad.obs["g2"] = g2
        got = cnv.tl.ithcna(ad, "g2", inplace=False)
        exp = O.ith_score(X.astype(np.float64), list(g2))
        for g in ("even", "odd"):
            assert (np.isnan(got[g]) and np.isnan(exp[g])) or abs(got[g] - exp[g]) <= 1e-5, desc + f" ithcna {g}: {got[g]} vs {exp[g]}"
    return desc + ("" if same_sizes or dup else " SIZES-DIFFER")


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    bad = []
    t0 = time.time()
    for seed in range(first, first + n):
        try:
            d = one_case(seed)
            if os.environ.get("FUZZ_VERBOSE") or d.endswith("SIZES-DIFFER"):
                print(f"seed {seed} ok {d}", flush=True)
        except Exception as e:  # noqa: BLE001 -- report and go on
            bad.append(seed)
            print(f"seed {seed}: {type(e).__name__}: {str(e)[:700]}", flush=True)
    print(f"fuzz ward: seeds {first}..{first + n - 1}: {n - len(bad)} passed, {len(bad)} failed {bad} "
          f"({time.time() - t0:.0f} s)", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

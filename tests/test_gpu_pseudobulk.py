"""tl.cnv_pseudobulk on the GPU equals the oracle of DESIGN.md 4.17 (tests/_pseudobulk_oracle.py) on the float64 bytes for
every kind of input, leaves device input on the device, fills the container as documented, and the HMM family runs on the
container: the planted clones that the vote of per-cell calls misses are called from the clone means."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _fit_oracle as fo
import _posterior_oracle as po
import _pseudobulk_oracle as pb
import _segments_oracle as sg
import _states_oracle as so

pytestmark = pytest.mark.gpu

SIZES = {"a": 129, "unused": 0, "c": 1, "d": 170, "e": 2}  # with min_cells=2: "unused" and "c" are dropped
LENGTHS = [150, 1, 182]  # W = 333


def _adata(x, chr_pos, labels, name="clone"):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32), obs=pd.DataFrame({name: labels}))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


@functools.lru_cache(maxsize=None)
def kinds_case():
    """Cells of five groups (one unused category) and 20 cells without a label, in shuffled order; float32 numbers, so
    that every kind of input holds the same values.  The oracle's result for min_cells=2 is computed once."""
    rng = np.random.default_rng(8)
    names = list(SIZES)
    codes = np.concatenate([np.full(SIZES[k], g) for g, k in enumerate(names)] + [np.full(20, -1)])
    rng.shuffle(codes)
    w = sum(LENGTHS)
    x = pb.random_sparse(codes.shape[0], w, 0.15, 9, dtype=np.float32).astype(np.float64)
    x.data[:5] = [0.0, -0.0, 700.5, -1023.0, 2.0 ** -60]
    kept = [g for g, k in enumerate(names) if SIZES[k] >= 2]
    remap = np.full(len(names) + 1, -1)
    remap[kept] = np.arange(len(kept))
    want = pb.profiles(x, remap[codes], len(kept))
    assert want["shift"] == 40 and want["n_cells"].tolist() == [129, 170, 2]
    return {"x": x, "labels": pd.Categorical.from_codes(codes, categories=names), "codes": codes, "names": names,
            "chr_pos": so.chr_pos_of(LENGTHS), "want": want}


def _inputs(x):
    import torch

    import infercnvpy_amd as cnv

    dense32 = x.toarray().astype(np.float32)
    packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), torch.from_numpy(x.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(x.data).cuda(), x.shape[1])
    return {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
            "dense_float64": dense32.astype(np.float64), "cuda_float32": torch.from_numpy(dense32).cuda(),
            "cuda_float64": torch.from_numpy(dense32.astype(np.float64)).cuda(), "packed_csr": packed}


def test_every_input_kind_gives_the_oracles_bytes_and_device_input_stays_on_the_device():
    import torch

    import infercnvpy_amd as cnv

    c = kinds_case()
    want = c["want"]
    assert (want["N"] > 0).any() and (want["mean"] != 0).any()
    for name, x in _inputs(c["x"]).items():
        ad = _adata(x, c["chr_pos"], c["labels"])
        clones, info = cnv.tl.cnv_pseudobulk(ad, "clone", min_cells=2, return_info=True)
        mean, fraction = clones.obsm["X_cnv"], clones.obsm["X_cnv_fraction"]
        assert clones.X is mean, name
        if name.startswith(("cuda", "packed")):
            for t in (mean, fraction):
                assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64, name
            mean, fraction = mean.cpu().numpy(), fraction.cpu().numpy()
        assert isinstance(mean, np.ndarray) and mean.dtype == np.float64 and fraction.dtype == np.float64, name
        assert mean.shape == (3, 333) and mean.tobytes() == want["mean"].tobytes(), name
        assert fraction.tobytes() == want["fraction"].tobytes(), name
        assert info["n_groups"] == 3 and info["shift"] == 40 and set(info["stage_ms"]) == {"profiles"}, name
        # adata is not modified
        assert ad.obsm["X_cnv"] is x and set(ad.obsm) == {"X_cnv"} and set(ad.uns) == {"cnv"} and list(ad.obs.columns) == ["clone"]


def test_the_container_is_as_documented():
    import infercnvpy_amd as cnv

    c = kinds_case()
    ad = _adata(c["x"], c["chr_pos"], c["labels"])
    clones = cnv.tl.cnv_pseudobulk(ad, "clone", min_cells=2)
    assert isinstance(clones, cnv.SimpleAnnData) and clones.shape == (3, 333)
    assert set(clones.obsm) == {"X_cnv", "X_cnv_fraction"} and set(clones.uns) == {"cnv", "cnv_pseudobulk"}
    assert clones.uns["cnv"] == {"chr_pos": c["chr_pos"]} and clones.uns["cnv"]["chr_pos"] is not ad.uns["cnv"]["chr_pos"]
    assert clones.uns["cnv_pseudobulk"] == {"groupby": "clone", "use_rep": "cnv", "shift": 40, "dropped": ["unused", "c"]}
    assert list(clones.obs.index) == ["a", "d", "e"] and list(clones.obs.columns) == ["clone", "n_cells"]
    assert clones.obs["n_cells"].dtype == np.int64 and clones.obs["n_cells"].tolist() == [129, 170, 2]
    assert isinstance(clones.obs["clone"].dtype, pd.CategoricalDtype)
    assert list(clones.obs["clone"].cat.categories) == c["names"] and clones.obs["clone"].tolist() == ["a", "d", "e"]
    # a plain column: groups in order of appearance, a missing label in no group, labels of any type
    plain = np.where(c["codes"] < 0, -1, c["codes"] * 10).astype(object)
    plain[plain == -1] = None
    ad = _adata(c["x"], c["chr_pos"], plain, name="cnv_leiden")
    clones = cnv.tl.cnv_pseudobulk(ad)
    codes2, uniques = pd.factorize(plain, use_na_sentinel=True)
    want = pb.profiles(c["x"], codes2, len(uniques))
    assert clones.X.tobytes() == want["mean"].tobytes() and clones.uns["cnv_pseudobulk"]["dropped"] == []
    assert list(clones.obs.index) == [str(v) for v in uniques] and clones.obs["cnv_leiden"].tolist() == list(uniques)
    assert clones.obs["n_cells"].tolist() == want["n_cells"].tolist() and not isinstance(clones.obs["cnv_leiden"].dtype,
                                                                                        pd.CategoricalDtype)
    # the other representation of the same adata
    ad.obsm["X_other"] = c["x"].toarray()
    ad.uns["other"] = {"chr_pos": {"only": 0}}
    clones = cnv.tl.cnv_pseudobulk(ad, use_rep="other")
    assert set(clones.obsm) == {"X_other", "X_other_fraction"} and clones.uns["other"] == {"chr_pos": {"only": 0}}
    assert clones.obsm["X_other"].tobytes() == want["mean"].tobytes()


def test_the_heatmap_draws_the_container():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import infercnvpy_amd as cnv

    c = kinds_case()
    clones = cnv.tl.cnv_pseudobulk(_adata(c["x"], c["chr_pos"], c["labels"]), "clone", min_cells=2)
    cnv.pl.chromosome_heatmap(clones, groupby="clone", show=False)
    matplotlib.pyplot.close("all")


# ---- the planted clones ----------------------------------------------------------------------------------------------------------
def test_planted_clones_are_called_from_the_container_and_missed_by_the_vote():
    """3 clones x 48 cells, noise 0.5, a shift of 0.3 over 145 of the 810 windows: tl.cnv_states on the container calls
    the truth exactly (0 wrong, as the oracles on the CPU), the consensus of the per-cell calls misses every altered
    window (145 wrong on the CPU); then each of the other HMM functions runs once on the container against its oracle."""
    import infercnvpy_amd as cnv

    c = pb.planted_clones()
    chr_pos = so.chr_pos_of(c["lengths"])
    labels = pd.Categorical.from_codes(c["codes"], categories=["clone0", "clone1", "clone2"])
    ad = _adata(c["x"], chr_pos, labels)
    want = pb.profiles(c["x"], c["codes"], 3)
    want_calls, want_fraction, want_params = so.cnv_states(want["mean"], chr_pos)
    assert int((want_calls != c["truth"]).sum()) == 0

    clones = cnv.tl.cnv_pseudobulk(ad, "clone")
    assert list(clones.obs.index) == ["clone0", "clone1", "clone2"] and clones.X.tobytes() == want["mean"].tobytes()
    cnv.tl.cnv_states(clones)
    calls = clones.obsm["X_cnv_states"]
    assert np.array_equal(calls, c["truth"]) and calls.tobytes() == want_calls.tobytes()
    assert np.asarray(clones.obs["cnv_states_fraction"]).tobytes() == want_fraction.tobytes()
    assert repr(clones.uns["cnv_states"]["params"]) == repr(want_params)

    # the vote of the per-cell calls: not the truth
    cnv.tl.cnv_states(ad)
    _, consensus, _, _ = cnv.tl.cnv_segments(ad, "clone", inplace=False)
    per_cell, _, _ = so.cnv_states(c["x"], chr_pos)
    want_consensus = sg.group_segments(per_cell, c["codes"], 3, sg.bounds(chr_pos, 270))["consensus"]
    assert np.array_equal(consensus, want_consensus) and not np.array_equal(consensus, c["truth"])
    missed = (consensus != c["truth"]) & (c["truth"] != 0)
    print(f"vote consensus: {int((consensus != c['truth']).sum())} of 810 wrong, {int(missed.sum())} of 145 altered missed")
    assert int(missed.sum()) == 145

    # the rest of the family, once each, on the container
    fitted = cnv.tl.cnv_states_fit(clones, inplace=False)
    assert repr(fitted) == repr(fo.cnv_states_fit(want["mean"], chr_pos)["params"])
    cnv.tl.cnv_posteriors(clones)
    _, neutral, _, _ = po.cnv_posteriors(want["mean"], chr_pos)
    assert clones.obsm["X_cnv_posterior_neutral"].tobytes() == neutral.tobytes()
    cnv.tl.cnv_states_filter(clones)
    filtered, _, removed = po.states_filter(want_calls, neutral, chr_pos)
    assert clones.obsm["X_cnv_states_filtered"].tobytes() == filtered.tobytes()
    assert np.array_equal(np.asarray(clones.obs["cnv_states_filtered_removed"]), removed)
    table = cnv.tl.cnv_segments(clones, inplace=False)
    runs = sg.segments(want_calls, sg.bounds(chr_pos, 270))
    assert len(table) == 3 and np.array_equal(table["cell"].to_numpy(), runs["row"])
    assert (table["start"].tolist(), table["end"].tolist(), table["state"].tolist()) == ([20, 130, 225], [70, 190, 260], [1, -1, 1])

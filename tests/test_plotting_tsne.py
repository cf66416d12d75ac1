"""pl.tsne, and pl.umap after the two were factored into one scatter routine (CPU, matplotlib's Agg backend)."""
import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import pytest  # noqa: E402

import infercnvpy_amd as cnv  # noqa: E402
from infercnvpy_amd._compat import SimpleAnnData  # noqa: E402


def _adata(n=60):
    rng = np.random.default_rng(0)
    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32))
    ad.obs["cnv_leiden"] = pd.Categorical.from_codes(np.arange(n) % 4, categories=["0", "1", "2", "3"])
    ad.obs["cnv_score"] = np.linspace(0, 1, n)
    ad.obs["flag"] = np.arange(n) % 2 == 0
    ad.obsm["X_cnv_tsne"] = rng.normal(size=(n, 2)).astype(np.float32)
    ad.obsm["X_cnv_umap"] = rng.normal(size=(n, 2)).astype(np.float32)
    return ad


def _describe(ax):
    pts = ax.collections[0]
    legend = ax.get_legend()
    return {"offsets": np.asarray(pts.get_offsets()).tolist(), "colors": np.asarray(pts.get_facecolors()).tolist(),
            "sizes": np.asarray(pts.get_sizes()).tolist(), "title": ax.get_title(),
            "xticks": list(ax.get_xticks()), "yticks": list(ax.get_yticks()),
            "legend": None if legend is None else ([t.get_text() for t in legend.get_texts()],
                                                   legend.get_title().get_text()),
            "n_axes": len(ax.figure.axes)}


def test_pl_tsne():
    ad = _adata()
    try:
        ax = cnv.pl.tsne(ad, color="cnv_leiden", s=3)
        assert np.array_equal(np.asarray(ax.collections[0].get_offsets()), ad.obsm["X_cnv_tsne"].astype(np.float64))
        assert [t.get_text() for t in ax.get_legend().get_texts()] == ["0", "1", "2", "3"]
        assert (ax.get_xlabel(), ax.get_ylabel(), ax.get_title()) == ("cnv_tsne1", "cnv_tsne2", "cnv_leiden")
        n_axes = len(ax.figure.axes)
        ax2 = cnv.pl.tsne(ad, color="cnv_score")
        assert len(ax2.figure.axes) == n_axes + 1 and ax2.get_legend() is None  # the colour bar
        _, own = plt.subplots()
        assert cnv.pl.tsne(ad, ax=own, show=False) is own and len(own.collections[0].get_offsets()) == 60
    finally:
        plt.close("all")


def test_pl_tsne_errors():
    ad = _adata()
    del ad.obsm["X_cnv_tsne"]
    with pytest.raises(KeyError, match="X_cnv_tsne.*Did you run `tl.tsne`"):
        cnv.pl.tsne(ad)
    with pytest.raises(KeyError, match="nope"):
        cnv.pl.tsne(_adata(), color="nope")


@pytest.mark.parametrize("color", (None, "cnv_leiden", "cnv_score", "flag"))
def test_pl_umap_draws_what_it_drew_before(color):
    """pl.umap is pl.tsne's routine on the other basis: on the same coordinates both draw the same picture, and
    pl.umap keeps its labels and its message."""
    ad = _adata()
    ad.obsm["X_cnv_tsne"] = ad.obsm["X_cnv_umap"]
    try:
        a = cnv.pl.umap(ad, color=color)
        b = cnv.pl.tsne(ad, color=color)
        assert _describe(a) == _describe(b)
        assert (a.get_xlabel(), a.get_ylabel()) == ("cnv_umap1", "cnv_umap2")
        assert a.get_title() == ("" if color is None else color)
        assert np.array_equal(np.asarray(a.collections[0].get_offsets()), ad.obsm["X_cnv_umap"].astype(np.float64))
        assert _describe(a)["sizes"] == [max(120000.0 / 60, 1.0) / 10.0] and _describe(a)["xticks"] == []
    finally:
        plt.close("all")
    del ad.obsm["X_cnv_umap"]
    with pytest.raises(KeyError, match="'X_cnv_umap' is not in `adata.obsm`. Did you run `tl.umap`\\?"):
        cnv.pl.umap(ad)

"""``pl.umap`` / ``pl.tsne`` (reference src/infercnvpy/pl/__init__.py:7-20): scatter plots of the CNV layouts.

The reference forwards to ``scanpy.pl.embedding(adata, "cnv_umap" / "cnv_tsne", ...)``; scanpy is not a dependency of
this package, so an equivalent matplotlib scatter is drawn directly.
"""
from __future__ import annotations

import numpy as np


def _scatter(adata, basis, tool, color, ax, show, scatter_kwargs):
    """The scatter plot of ``adata.obsm[f"X_{basis}"]`` (written by ``tool``); see :func:`umap` for the arguments."""
    if f"X_{basis}" not in adata.obsm:
        raise KeyError(f"'X_{basis}' is not in `adata.obsm`. Did you run `{tool}`?")
    if color is not None and color not in adata.obs.columns:
        raise KeyError(f"{color!r} is not a column of `adata.obs`")
    import matplotlib.pyplot as plt
    import pandas as pd

    y = np.asarray(adata.obsm[f"X_{basis}"])
    if ax is None:
        _, ax = plt.subplots(figsize=(6, 6))
    scatter_kwargs.setdefault("s", max(120000.0 / max(len(y), 1), 1.0) / 10.0)
    scatter_kwargs.setdefault("linewidths", 0)
    if color is None:
        ax.scatter(y[:, 0], y[:, 1], **scatter_kwargs)
    else:
        col = adata.obs[color]
        if pd.api.types.is_numeric_dtype(col.dtype) and not pd.api.types.is_bool_dtype(col.dtype):
            pts = ax.scatter(y[:, 0], y[:, 1], c=np.asarray(col, dtype=np.float64), **scatter_kwargs)
            ax.figure.colorbar(pts, ax=ax, label=color)
        else:
            cat = col if isinstance(col.dtype, pd.CategoricalDtype) else col.astype("category")
            codes = np.asarray(cat.cat.codes)
            cats = list(cat.cat.categories)
            cmap = plt.get_cmap(scatter_kwargs.pop("cmap", "tab20"))
            colours = np.array([cmap(i % cmap.N) for i in range(max(len(cats), 1))])
            rgba = np.where((codes >= 0)[:, None], colours[np.maximum(codes, 0)], (0.8, 0.8, 0.8, 1.0))
            ax.scatter(y[:, 0], y[:, 1], c=rgba, **scatter_kwargs)
            handles = [plt.Line2D([], [], marker="o", ls="", color=colours[i], label=str(name))
                       for i, name in enumerate(cats)]
            ax.legend(handles=handles, title=color, loc="center left", bbox_to_anchor=(1.0, 0.5), frameon=False,
                      ncol=1 + len(cats) // 20)
        ax.set_title(color)
    ax.set_xlabel(f"{basis}1")
    ax.set_ylabel(f"{basis}2")
    ax.set_xticks([])
    ax.set_yticks([])
    if show:
        plt.show()
        return None
    return ax


def umap(adata, color=None, *, ax=None, show=None, **scatter_kwargs):
    """Plot the CNV UMAP (``adata.obsm["X_cnv_umap"]``, written by :func:`infercnvpy_amd.tl.umap`).

    Parameters
    ----------
    color
        A column of ``adata.obs``: a categorical (or string / boolean) column gives one colour per category and a
        legend, a numeric one a colour bar.  None: one colour.
    ax
        Axes to draw into (a new figure otherwise).
    show
        True: ``matplotlib.pyplot.show()`` and return None; otherwise the axes are returned.
    scatter_kwargs
        Passed to ``Axes.scatter`` (``s``, ``alpha``, ``cmap``, ...).
    """
    return _scatter(adata, "cnv_umap", "tl.umap", color, ax, show, scatter_kwargs)


def tsne(adata, color=None, *, ax=None, show=None, **scatter_kwargs):
    """Plot the CNV t-SNE (``adata.obsm["X_cnv_tsne"]``, written by :func:`infercnvpy_amd.tl.tsne`); the arguments of
    :func:`umap`."""
    return _scatter(adata, "cnv_tsne", "tl.tsne", color, ax, show, scatter_kwargs)

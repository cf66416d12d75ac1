from ._chromosome_heatmap import chromosome_heatmap, chromosome_heatmap_summary
from ._embedding import tsne, umap

__all__ = ["chromosome_heatmap", "chromosome_heatmap_summary", "umap", "tsne"]

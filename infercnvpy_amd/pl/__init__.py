from ._chromosome_heatmap import chromosome_heatmap, chromosome_heatmap_summary
from ._embedding import umap

__all__ = ["chromosome_heatmap", "chromosome_heatmap_summary", "umap"]

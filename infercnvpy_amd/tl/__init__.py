from ._changepoints import cnv_changepoints
from ._copy_fit import cnv_copy_states_fit
from ._copy_posteriors import cnv_copy_posteriors, cnv_copy_states_filter
from ._copy_segments import cnv_copy_segments
from ._copy_states import cnv_copy_states
from ._correlation import cnv_correlation, cnv_signal
from ._fit import cnv_states_fit
from ._infercnv import infercnv, infercnv_device
from ._leiden import leiden
from ._pca import pca
from ._tsne import tsne
from ._umap import umap
from ._linkage import cell_linkage, leaves_list, ward_linkage
from ._pool import cnv_pool_neighbors
from ._posteriors import cnv_posteriors, cnv_states_filter
from ._pseudobulk import cnv_pseudobulk
from ._rank import cnv_rank_groups
from ._scores import cnv_score, ithcna, ithgex
from ._segments import cnv_segments
from ._kmeans import cnv_kmeans
from ._silhouette import cnv_silhouette
from ._states import cnv_states

__all__ = ["infercnv", "infercnv_device", "pca", "leiden", "umap", "tsne", "cnv_score", "cnv_states", "cnv_copy_states", "cnv_states_fit", "cnv_segments", "cnv_pseudobulk", "cnv_pool_neighbors", "cnv_rank_groups", "cnv_correlation", "cnv_signal", "cnv_changepoints", "cnv_posteriors", "cnv_states_filter", "cnv_copy_posteriors", "cnv_copy_states_filter", "cnv_copy_states_fit", "cnv_copy_segments", "cnv_silhouette", "cnv_kmeans", "ithcna", "ithgex", "cell_linkage", "ward_linkage", "leaves_list"]

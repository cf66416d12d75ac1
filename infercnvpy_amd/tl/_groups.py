"""The groups of a label column, for ``tl.cnv_score``, ``tl.cnv_segments`` and ``tl.cnv_pseudobulk``: the group number of
every cell, and the lists of each group's rows that the device kernels read."""
from __future__ import annotations

import numpy as np


def group_codes(adata, groupby):
    """(codes int64 n, labels of the G groups) of ``adata.obs[groupby]``: the categories of a categorical column (an
    unused one is a group of no cells), otherwise the distinct values in order of appearance; -1 is a missing label."""
    import pandas as pd

    labels = adata.obs[groupby]
    if isinstance(getattr(labels, "dtype", None), pd.CategoricalDtype):
        codes, uniques = labels.cat.codes.to_numpy(), labels.cat.categories
    else:
        codes, uniques = pd.factorize(np.asarray(labels.values if hasattr(labels, "values") else labels),
                                      use_na_sentinel=True)
    return np.asarray(codes, dtype=np.int64), np.asarray(uniques)


def group_table(codes, n_groups, keep=None, sizes=None):
    """(rows, group_ptr, sizes), int64: the row numbers of the cells with a code >= 0 sorted by group (ascending inside a
    group), the G + 1 positions of the groups in ``rows`` and the G group sizes.  ``keep``: the ascending numbers of the
    groups to list; they are renumbered 0 .. len(keep) - 1 and the cells of the others belong to no group.  ``sizes``: the
    int64 sizes of all ``n_groups`` groups, where the caller has counted them already."""
    if sizes is None:
        sizes = np.bincount(codes[codes >= 0], minlength=n_groups).astype(np.int64)
    if keep is not None:
        new_code = np.full(n_groups + 1, -1, dtype=np.int64)  # (the last slot takes the code -1)
        new_code[keep] = np.arange(len(keep))
        codes, sizes = new_code[codes], sizes[keep]
    rows = np.argsort(codes, kind="stable")[codes.shape[0] - int(sizes.sum()):].astype(np.int64)  # (-1 sorts first)
    group_ptr = np.zeros(sizes.shape[0] + 1, dtype=np.int64)
    group_ptr[1:] = np.cumsum(sizes)
    return rows, group_ptr, sizes

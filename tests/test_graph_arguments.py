"""The arguments of tl.leiden, tl.umap and tl.tsne that are refused before any GPU work: for every bad input the
exception's type and its whole message.  The three functions share the intake of the graph, the checks of n_components
and random_state, the initial positions and the tail (tl/_graph.py); the strings below are what each function raised
when it still had its own copy, so the table holds the shared helpers to them character for character.  An input that
is wrong in two ways is listed with the fault that was reported then.  No test here needs a device."""
import numpy as np
import pytest
import scipy.sparse as sp

N_GRAPH, N_POINTS = 6, 40  # cells of the tl.leiden / tl.umap cases, points of the tl.tsne cases


def _ring(n=N_GRAPH):
    i = np.arange(n)
    a = sp.coo_matrix((np.full(n, 0.5, dtype=np.float32), (i, (i + 1) % n)), shape=(n, n))
    return sp.csr_matrix(a + a.T)


def _graph_adata(**obsm):
    """6 cells, the ring under the keys pp.neighbors writes, a second graph under obsp['other']."""
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((N_GRAPH, 3), dtype=np.float32))
    ad.obsp["cnv_neighbors_connectivities"] = _ring()
    ad.obsp["other"] = _ring()
    ad.uns["cnv_neighbors"] = {"connectivities_key": "cnv_neighbors_connectivities"}
    ad.uns["dangling"] = {"connectivities_key": "gone"}
    ad.obsm.update(obsm)
    return ad


def _points_adata(**obsm):
    """40 points in 5 dimensions under obsm['X_cnv_pca']."""
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((N_POINTS, 3), dtype=np.float32))
    ad.obsm["X_cnv_pca"] = np.random.default_rng(0).standard_normal((N_POINTS, 5)).astype(np.float32)
    ad.obsm.update(obsm)
    return ad


def _nan(shape):
    a = np.zeros(shape, dtype=np.float32)
    a[1, 1] = np.nan
    return a


def _graph_cases(fn):
    """The bad inputs tl.leiden and tl.umap have in common."""
    return [
        ("unknown keyword", _graph_adata, {"bogus": 1, "extra": 2}),
        ("random_state=0.5", _graph_adata, {"random_state": 0.5}),
        ("random_state='x'", _graph_adata, {"random_state": "x"}),
        ("missing neighbors_key", _graph_adata, {"neighbors_key": "nope"}),
        ("missing connectivities", _graph_adata, {"neighbors_key": "dangling"}),
        ("missing obsp key", _graph_adata, {"obsp": "nope"}),
        ("non-square adjacency", _graph_adata, {"adjacency": sp.csr_matrix((6, 5))}),
        ("empty adjacency", _graph_adata, {"adjacency": sp.csr_matrix((0, 0))}),
        ("dense adjacency", _graph_adata, {"adjacency": np.zeros((6, 6))}),
        ("5 vertices on 6 cells", _graph_adata, {"adjacency": _ring(5)}),
        ("random_state=0.5 and a missing key", _graph_adata, {"random_state": 0.5, "obsp": "nope"}),
        ("adjacency before a missing obsp key", _graph_adata, {"obsp": "nope", "adjacency": _ring(5)}),
    ]


def _init_cases(make, named_key):
    """The bad initial positions tl.umap (6 cells) and tl.tsne (40 points) have in common."""
    n = N_GRAPH if make is _graph_adata else N_POINTS
    return [
        ("init_pos unknown key", make, {"init_pos": "nope"}),
        ("init_pos wrong shape", make, {"init_pos": np.zeros((n, 3), dtype=np.float32)}),
        ("init_pos wrong rows", make, {"init_pos": np.zeros((n + 1, 2), dtype=np.float32)}),
        ("init_pos NaN", make, {"init_pos": _nan((n, 2))}),
        ("init_pos key wrong shape", lambda: make(X_start=np.zeros((n, 2))), {"init_pos": "X_start", "n_components": 3}),
        ("init_pos key NaN", lambda: make(X_start=_nan((n, 2))), {"init_pos": "X_start"}),
        (f"init_pos={named_key!r}", make, {"init_pos": named_key}),
    ]


def _components_cases(make):
    return [(f"n_components={v!r}", make, {"n_components": v}) for v in (1, 4, 2.5, "2", True)]


def _cases(fn):
    """(id, () -> adata, keywords) of every bad input of the function ``fn``."""
    if fn == "leiden":
        return _graph_cases(fn) + [
            ("resolution='x'", _graph_adata, {"resolution": "x"}),
            ("resolution=-1", _graph_adata, {"resolution": -1}),
            ("resolution=nan", _graph_adata, {"resolution": float("nan")}),
            ("resolution=inf", _graph_adata, {"resolution": float("inf")}),
            ("n_iterations=0", _graph_adata, {"n_iterations": 0}),
            ("n_iterations=-2", _graph_adata, {"n_iterations": -2}),
            ("n_iterations=2.5", _graph_adata, {"n_iterations": 2.5}),
            ("n_iterations='x'", _graph_adata, {"n_iterations": "x"}),
            ("resolution and n_iterations", _graph_adata, {"resolution": -1, "n_iterations": 0}),
            ("n_iterations and random_state", _graph_adata, {"n_iterations": 0, "random_state": 0.5}),
            ("unknown keyword and resolution", _graph_adata, {"bogus": 1, "resolution": -1}),
        ]
    if fn == "umap":
        return _graph_cases(fn) + _components_cases(_graph_adata) + [
            ("negative_sample_rate=65", _graph_adata, {"negative_sample_rate": 65}),
            ("negative_sample_rate=-1", _graph_adata, {"negative_sample_rate": -1}),
            ("negative_sample_rate=2.5", _graph_adata, {"negative_sample_rate": 2.5}),
            ("negative_sample_rate='x'", _graph_adata, {"negative_sample_rate": "x"}),
            ("alpha='x'", _graph_adata, {"alpha": "x"}),
            ("alpha=-1", _graph_adata, {"alpha": -1}),
            ("gamma=nan", _graph_adata, {"gamma": float("nan")}),
            ("min_dist=None", _graph_adata, {"min_dist": None}),
            ("spread='x'", _graph_adata, {"spread": "x"}),
            ("a without b", _graph_adata, {"a": 1.0}),
            ("b without a", _graph_adata, {"b": 1.0}),
            ("min_dist=-1", _graph_adata, {"min_dist": -1}),
            ("spread=0", _graph_adata, {"spread": 0}),
            ("spread=inf", _graph_adata, {"spread": float("inf")}),
            ("a=-1", _graph_adata, {"a": -1, "b": 1}),
            ("b=inf", _graph_adata, {"a": 1, "b": float("inf")}),
            ("maxiter=0", _graph_adata, {"maxiter": 0}),
            ("maxiter=2.5", _graph_adata, {"maxiter": 2.5}),
        ] + _init_cases(_graph_adata, "pca") + [
            ("n_components and random_state", _graph_adata, {"n_components": 4, "random_state": 0.5}),
            ("random_state and negative_sample_rate", _graph_adata, {"random_state": 0.5, "negative_sample_rate": 65}),
            ("a without b and a missing key", _graph_adata, {"a": 1.0, "obsp": "nope"}),
            ("5 vertices and maxiter", _graph_adata, {"adjacency": _ring(5), "maxiter": 0}),
            ("maxiter and init_pos", _graph_adata, {"maxiter": 0, "init_pos": "nope"}),
        ]
    return [
        ("unknown keyword", _points_adata, {"bogus": 1, "extra": 2}),
        ("random_state=0.5", _points_adata, {"random_state": 0.5}),
        ("random_state='x'", _points_adata, {"random_state": "x"}),
    ] + _components_cases(_points_adata) + [
        ("perplexity='x'", _points_adata, {"perplexity": "x"}),
        ("perplexity=0", _points_adata, {"perplexity": 0}),
        ("perplexity=nan", _points_adata, {"perplexity": float("nan")}),
        ("early_exaggeration=0", _points_adata, {"early_exaggeration": 0}),
        ("early_exaggeration=None", _points_adata, {"early_exaggeration": None}),
        ("learning_rate=-1", _points_adata, {"learning_rate": -1}),
        ("learning_rate=inf", _points_adata, {"learning_rate": float("inf")}),
        ("max_iter=-1", _points_adata, {"max_iter": -1}),
        ("max_iter=2.5", _points_adata, {"max_iter": 2.5}),
        ("missing X_other", _points_adata, {"use_rep": "other"}),
        ("1-D representation", _points_adata, {"use_rep": np.zeros(N_POINTS, dtype=np.float32)}),
        ("NaN representation", _points_adata, {"use_rep": _nan((N_POINTS, 5))}),
        ("n_pcs=0", _points_adata, {"n_pcs": 0}),
        ("n_pcs=6", _points_adata, {"n_pcs": 6}),
        ("n_pcs=2.5", _points_adata, {"n_pcs": 2.5}),
        ("300 columns", _points_adata, {"use_rep": np.zeros((N_POINTS, 300), dtype=np.float32)}),
        ("perplexity=39", _points_adata, {"perplexity": 39}),
        ("perplexity=50", _points_adata, {"perplexity": 50}),
        ("perplexity=0.2", _points_adata, {"perplexity": 0.2}),
    ] + _init_cases(_points_adata, "spectral") + [
        ("init_pos='pca' of one column", _points_adata, {"n_pcs": 1}),
        ("init_pos='pca' of a constant column", _points_adata, {"use_rep": np.ones((N_POINTS, 5), dtype=np.float32)}),
        ("n_components and random_state", _points_adata, {"n_components": 4, "random_state": 0.5}),
        ("random_state and perplexity", _points_adata, {"random_state": 0.5, "perplexity": 0}),
        ("perplexity and max_iter", _points_adata, {"perplexity": 0, "max_iter": -1}),
        ("max_iter and a missing key", _points_adata, {"max_iter": -1, "use_rep": "other"}),
        ("n_pcs and perplexity", _points_adata, {"n_pcs": 0, "perplexity": 50}),
        ("perplexity and init_pos", _points_adata, {"perplexity": 50, "init_pos": "nope"}),
    ]


# what the functions raised before tl/_graph.py existed
EXPECTED = {
    "leiden": {
        'unknown keyword': (ValueError, 'tl.leiden: unsupported keyword argument(s): bogus, extra'),
        'random_state=0.5': (ValueError, 'tl.leiden: random_state=0.5 is not an integer'),
        "random_state='x'": (ValueError, 'tl.leiden: n_iterations and random_state must be integers'),
        'missing neighbors_key': (KeyError, "'nope' is not in adata.uns. Did you run `pp.neighbors`?"),
        'missing connectivities': (KeyError, "'gone' is not in adata.obsp. Did you run `pp.neighbors`?"),
        'missing obsp key': (KeyError, "'nope' is not in adata.obsp. Did you run `pp.neighbors`?"),
        'non-square adjacency': (ValueError, 'tl.leiden: the adjacency matrix must be square'),
        'empty adjacency': (ValueError, 'tl.leiden: the adjacency matrix is empty'),
        'dense adjacency': (ValueError, 'tl.leiden: the graph must be a scipy sparse matrix or (indptr, indices, data) CUDA tensors'),
        '5 vertices on 6 cells': (ValueError, 'tl.leiden: the graph has 5 vertices, adata has 6 cells'),
        'random_state=0.5 and a missing key': (ValueError, 'tl.leiden: random_state=0.5 is not an integer'),
        'adjacency before a missing obsp key': (ValueError, 'tl.leiden: the graph has 5 vertices, adata has 6 cells'),
        "resolution='x'": (ValueError, "tl.leiden: resolution='x' is not a number"),
        'resolution=-1': (ValueError, 'tl.leiden: resolution=-1 must be a finite number >= 0'),
        'resolution=nan': (ValueError, 'tl.leiden: resolution=nan must be a finite number >= 0'),
        'resolution=inf': (ValueError, 'tl.leiden: resolution=inf must be a finite number >= 0'),
        'n_iterations=0': (ValueError, 'tl.leiden: n_iterations=0 must be -1 or a positive integer'),
        'n_iterations=-2': (ValueError, 'tl.leiden: n_iterations=-2 must be -1 or a positive integer'),
        'n_iterations=2.5': (ValueError, 'tl.leiden: n_iterations=2.5 must be -1 or a positive integer'),
        "n_iterations='x'": (ValueError, 'tl.leiden: n_iterations and random_state must be integers'),
        'resolution and n_iterations': (ValueError, 'tl.leiden: resolution=-1 must be a finite number >= 0'),
        'n_iterations and random_state': (ValueError, 'tl.leiden: n_iterations=0 must be -1 or a positive integer'),
        'unknown keyword and resolution': (ValueError, 'tl.leiden: unsupported keyword argument(s): bogus'),
    },
    "umap": {
        'unknown keyword': (ValueError, 'tl.umap: unsupported keyword argument(s): bogus, extra'),
        'random_state=0.5': (ValueError, 'tl.umap: random_state=0.5 is not an integer'),
        "random_state='x'": (ValueError, 'tl.umap: random_state, negative_sample_rate, alpha, gamma, min_dist and spread must be numbers'),
        'missing neighbors_key': (KeyError, "'nope' is not in adata.uns. Did you run `pp.neighbors`?"),
        'missing connectivities': (KeyError, "'gone' is not in adata.obsp. Did you run `pp.neighbors`?"),
        'missing obsp key': (KeyError, "'nope' is not in adata.obsp. Did you run `pp.neighbors`?"),
        'non-square adjacency': (ValueError, 'tl.umap: the adjacency matrix must be square'),
        'empty adjacency': (ValueError, 'tl.umap: the adjacency matrix is empty'),
        'dense adjacency': (ValueError, 'tl.umap: the graph must be a scipy sparse matrix or (indptr, indices, data) CUDA tensors'),
        '5 vertices on 6 cells': (ValueError, 'tl.umap: the graph has 5 vertices, adata has 6 cells'),
        'random_state=0.5 and a missing key': (ValueError, 'tl.umap: random_state=0.5 is not an integer'),
        'adjacency before a missing obsp key': (ValueError, 'tl.umap: the graph has 5 vertices, adata has 6 cells'),
        'n_components=1': (ValueError, 'tl.umap: n_components=1 must be 2 or 3'),
        'n_components=4': (ValueError, 'tl.umap: n_components=4 must be 2 or 3'),
        'n_components=2.5': (ValueError, 'tl.umap: n_components=2.5 must be 2 or 3'),
        "n_components='2'": (ValueError, "tl.umap: n_components='2' must be 2 or 3"),
        'n_components=True': (ValueError, 'tl.umap: n_components=True must be 2 or 3'),
        'negative_sample_rate=65': (ValueError, 'tl.umap: negative_sample_rate=65 must be an integer in [0, 64]'),
        'negative_sample_rate=-1': (ValueError, 'tl.umap: negative_sample_rate=-1 must be an integer in [0, 64]'),
        'negative_sample_rate=2.5': (ValueError, 'tl.umap: negative_sample_rate=2.5 must be an integer in [0, 64]'),
        "negative_sample_rate='x'": (ValueError, 'tl.umap: random_state, negative_sample_rate, alpha, gamma, min_dist and spread must be numbers'),
        "alpha='x'": (ValueError, 'tl.umap: random_state, negative_sample_rate, alpha, gamma, min_dist and spread must be numbers'),
        'alpha=-1': (ValueError, 'tl.umap: alpha and gamma must be finite numbers >= 0'),
        'gamma=nan': (ValueError, 'tl.umap: alpha and gamma must be finite numbers >= 0'),
        'min_dist=None': (ValueError, 'tl.umap: random_state, negative_sample_rate, alpha, gamma, min_dist and spread must be numbers'),
        "spread='x'": (ValueError, 'tl.umap: random_state, negative_sample_rate, alpha, gamma, min_dist and spread must be numbers'),
        'a without b': (ValueError, 'tl.umap: give both a and b, or neither'),
        'b without a': (ValueError, 'tl.umap: give both a and b, or neither'),
        'min_dist=-1': (ValueError, 'tl.umap: min_dist must be >= 0 and spread > 0'),
        'spread=0': (ValueError, 'tl.umap: min_dist must be >= 0 and spread > 0'),
        'spread=inf': (ValueError, 'tl.umap: min_dist must be >= 0 and spread > 0'),
        'a=-1': (ValueError, 'tl.umap: a and b must be finite numbers > 0'),
        'b=inf': (ValueError, 'tl.umap: a and b must be finite numbers > 0'),
        'maxiter=0': (ValueError, 'tl.umap: maxiter=0 must be None or a positive integer'),
        'maxiter=2.5': (ValueError, 'tl.umap: maxiter=2.5 must be None or a positive integer'),
        'init_pos unknown key': (KeyError, "tl.umap: init_pos='nope' is neither 'spectral', 'random' nor a key of adata.obsm"),
        'init_pos wrong shape': (ValueError, 'tl.umap: init_pos has shape (6, 3), expected (6, 2)'),
        'init_pos wrong rows': (ValueError, 'tl.umap: init_pos has shape (7, 2), expected (6, 2)'),
        'init_pos NaN': (ValueError, 'tl.umap: init_pos has non-finite values'),
        'init_pos key wrong shape': (ValueError, 'tl.umap: init_pos has shape (6, 2), expected (6, 3)'),
        'init_pos key NaN': (ValueError, 'tl.umap: init_pos has non-finite values'),
        "init_pos='pca'": (KeyError, "tl.umap: init_pos='pca' is neither 'spectral', 'random' nor a key of adata.obsm"),
        'n_components and random_state': (ValueError, 'tl.umap: n_components=4 must be 2 or 3'),
        'random_state and negative_sample_rate': (ValueError, 'tl.umap: random_state=0.5 is not an integer'),
        'a without b and a missing key': (ValueError, 'tl.umap: give both a and b, or neither'),
        '5 vertices and maxiter': (ValueError, 'tl.umap: the graph has 5 vertices, adata has 6 cells'),
        'maxiter and init_pos': (ValueError, 'tl.umap: maxiter=0 must be None or a positive integer'),
    },
    "tsne": {
        'unknown keyword': (ValueError, 'tl.tsne: unsupported keyword argument(s): bogus, extra'),
        'random_state=0.5': (ValueError, 'tl.tsne: random_state=0.5 is not an integer'),
        "random_state='x'": (ValueError, 'tl.tsne: random_state, perplexity, early_exaggeration and learning_rate must be numbers'),
        'n_components=1': (ValueError, 'tl.tsne: n_components=1 must be 2 or 3'),
        'n_components=4': (ValueError, 'tl.tsne: n_components=4 must be 2 or 3'),
        'n_components=2.5': (ValueError, 'tl.tsne: n_components=2.5 must be 2 or 3'),
        "n_components='2'": (ValueError, "tl.tsne: n_components='2' must be 2 or 3"),
        'n_components=True': (ValueError, 'tl.tsne: n_components=True must be 2 or 3'),
        "perplexity='x'": (ValueError, 'tl.tsne: random_state, perplexity, early_exaggeration and learning_rate must be numbers'),
        'perplexity=0': (ValueError, 'tl.tsne: perplexity, early_exaggeration and learning_rate must be finite numbers > 0'),
        'perplexity=nan': (ValueError, 'tl.tsne: perplexity, early_exaggeration and learning_rate must be finite numbers > 0'),
        'early_exaggeration=0': (ValueError, 'tl.tsne: perplexity, early_exaggeration and learning_rate must be finite numbers > 0'),
        'early_exaggeration=None': (ValueError, 'tl.tsne: random_state, perplexity, early_exaggeration and learning_rate must be numbers'),
        'learning_rate=-1': (ValueError, 'tl.tsne: perplexity, early_exaggeration and learning_rate must be finite numbers > 0'),
        'learning_rate=inf': (ValueError, 'tl.tsne: perplexity, early_exaggeration and learning_rate must be finite numbers > 0'),
        'max_iter=-1': (ValueError, 'tl.tsne: max_iter=-1 must be a non-negative integer'),
        'max_iter=2.5': (ValueError, 'tl.tsne: max_iter=2.5 must be a non-negative integer'),
        'missing X_other': (KeyError, 'X_other is not in adata.obsm.'),
        '1-D representation': (ValueError, 'pp.neighbors: the representation must be 2-D'),
        'NaN representation': (ValueError, 'Input X contains NaN or infinity.'),
        'n_pcs=0': (ValueError, 'tl.tsne: n_pcs=0 must be an integer in [1, 5]'),
        'n_pcs=6': (ValueError, 'tl.tsne: n_pcs=6 must be an integer in [1, 5]'),
        'n_pcs=2.5': (ValueError, 'tl.tsne: n_pcs=2.5 must be an integer in [1, 5]'),
        '300 columns': (ValueError, 'tl.tsne: the representation has 300 columns; 1 .. 256 are supported'),
        'perplexity=39': (ValueError, 'tl.tsne: perplexity=39 must be less than the number of neighbours used, min(floor(3 perplexity), 63, n_obs - 1) = 39'),
        'perplexity=50': (ValueError, 'tl.tsne: perplexity=50 must be less than the number of neighbours used, min(floor(3 perplexity), 63, n_obs - 1) = 39'),
        'perplexity=0.2': (ValueError, 'tl.tsne: perplexity=0.2 must be less than the number of neighbours used, min(floor(3 perplexity), 63, n_obs - 1) = 0'),
        'init_pos unknown key': (KeyError, "tl.tsne: init_pos='nope' is neither 'pca', 'random' nor a key of adata.obsm"),
        'init_pos wrong shape': (ValueError, 'tl.tsne: init_pos has shape (40, 3), expected (40, 2)'),
        'init_pos wrong rows': (ValueError, 'tl.tsne: init_pos has shape (41, 2), expected (40, 2)'),
        'init_pos NaN': (ValueError, 'tl.tsne: init_pos has non-finite values'),
        'init_pos key wrong shape': (ValueError, 'tl.tsne: init_pos has shape (40, 2), expected (40, 3)'),
        'init_pos key NaN': (ValueError, 'tl.tsne: init_pos has non-finite values'),
        "init_pos='spectral'": (KeyError, "tl.tsne: init_pos='spectral' is neither 'pca', 'random' nor a key of adata.obsm"),
        "init_pos='pca' of one column": (ValueError, "tl.tsne: init_pos='pca' needs at least n_components=2 columns, the representation has 1"),
        "init_pos='pca' of a constant column": (ValueError, "tl.tsne: init_pos='pca' needs a first column that is not constant"),
        'n_components and random_state': (ValueError, 'tl.tsne: n_components=4 must be 2 or 3'),
        'random_state and perplexity': (ValueError, 'tl.tsne: random_state=0.5 is not an integer'),
        'perplexity and max_iter': (ValueError, 'tl.tsne: perplexity, early_exaggeration and learning_rate must be finite numbers > 0'),
        'max_iter and a missing key': (ValueError, 'tl.tsne: max_iter=-1 must be a non-negative integer'),
        'n_pcs and perplexity': (ValueError, 'tl.tsne: n_pcs=0 must be an integer in [1, 5]'),
        'perplexity and init_pos': (ValueError, 'tl.tsne: perplexity=50 must be less than the number of neighbours used, min(floor(3 perplexity), 63, n_obs - 1) = 39'),
    },
}


@pytest.mark.parametrize("fn", list(EXPECTED))
def test_every_bad_input_keeps_its_exception_and_its_whole_message(fn):
    import infercnvpy_amd as cnv

    cases = _cases(fn)
    assert [cid for cid, _, _ in cases] == list(EXPECTED[fn])
    for cid, make, kw in cases:
        kind, message = EXPECTED[fn][cid]
        with pytest.raises(kind) as info:
            getattr(cnv.tl, fn)(make(), **kw)
        assert type(info.value) is kind, (fn, cid)
        assert info.value.args[0] == message, (fn, cid)


def test_nothing_is_written_to_adata_by_a_refused_call():
    import infercnvpy_amd as cnv

    for fn, make in (("leiden", _graph_adata), ("umap", _graph_adata), ("tsne", _points_adata)):
        ad = make()
        keys = (set(ad.obs.columns), set(ad.obsm), set(ad.uns), set(ad.obsp))
        with pytest.raises(ValueError):
            getattr(cnv.tl, fn)(ad, random_state=0.5)
        assert (set(ad.obs.columns), set(ad.obsm), set(ad.uns), set(ad.obsp)) == keys


def test_the_helpers_have_one_home():
    from infercnvpy_amd.tl import _graph, _leiden, _tsne, _umap

    for name in ("_is_tensor", "_graph", "_host_csr"):  # (the first home of these three stays importable)
        assert getattr(_leiden, name) is getattr(_graph, name)
    assert _umap._uniform24 is _graph._uniform24 and _tsne._uniform24 is _graph._uniform24
    assert _umap.resolve_init is _tsne.resolve_init is _graph.resolve_init
    assert _umap.resolve_graph is _leiden.resolve_graph is _graph.resolve_graph
    assert _umap.random_init is not _tsne.random_init  # (each keeps its own distribution)

"""The arguments ``tl.infercnv`` (host matrix) and ``tl.infercnv_device`` refuse before a device is touched: for every
bad input the exception's type and its whole message, and for inputs with two faults which one is reported.  The host
path asks ``_engine._torch()`` for torch -- which refuses a machine without a GPU -- between its ``chunksize`` check and
its dtype / reference checks; the tests hand it the module itself so that those checks are reached without a device."""
import numpy as np
import pandas as pd
import pytest

import cases

MEAN_ORDER = "mean_order must be 'reference' (numpy's / scipy's evaluation order) or 'float64'"
CHUNKSIZE = "chunksize must be >= 1"
REFERENCE = "Reference must match the number of genes in AnnData. "
N_CELLS, GENES = 20, [30, 20, 10]


def _adata(dtype=np.float32, dup_names=False, drop=None):
    from infercnvpy_amd._compat import SimpleAnnData

    v = cases.synthetic_var(GENES)
    names = list(v["names"])
    if dup_names:
        names[1] = names[0]
    var = pd.DataFrame({"chromosome": v["chromosome"], "start": v["start"], "end": v["end"]}, index=names)
    if drop:
        var = var.drop(columns=drop)
    X = cases.synthetic_expr(N_CELLS, len(names), seed=8).astype(dtype)
    obs = pd.DataFrame({"group": np.array(["n", "t"])[np.arange(N_CELLS) % 2]})
    return SimpleAnnData(X, obs=obs, var=var)


N_GENES = sum(GENES)
# (id, keywords of _adata, keywords of tl.infercnv, exception type, whole message); two faults: the one reported today
FAULTS = [
    ("var_names", dict(dup_names=True), {}, ValueError, "Ensure your var_names are unique!"),
    ("no chromosome", dict(drop=["chromosome"]), {}, ValueError,
     "Genomic positions not found. There need to be `chromosome`, `start`, and `end` columns in `adata.var`. "),
    ("no start, no end", dict(drop=["start", "end"]), {}, ValueError,
     "Genomic positions not found. There need to be `chromosome`, `start`, and `end` columns in `adata.var`. "),
    ("mean_order", {}, dict(mean_order="numpy"), ValueError, MEAN_ORDER),
    ("mean_order None", {}, dict(mean_order=None), ValueError, MEAN_ORDER),
    ("chunksize 0", {}, dict(chunksize=0), ValueError, CHUNKSIZE),
    ("chunksize negative", {}, dict(chunksize=-5), ValueError, CHUNKSIZE),
    ("chunksize string", {}, dict(chunksize="x"), ValueError, "invalid literal for int() with base 10: 'x'"),
    ("complex matrix", dict(dtype=np.complex64), dict(reference=np.zeros(N_GENES, np.float32)), ValueError,
     "unsupported matrix dtype complex64"),
    ("absent category", {}, dict(reference_key="group", reference_cat=["n", "x", "y"]), ValueError,
     "The following reference categories were not found in adata.obs[reference_key]: ['x' 'y']"),
    ("absent category, string", {}, dict(reference_key="group", reference_cat="nope"), ValueError,
     "The following reference categories were not found in adata.obs[reference_key]: ['nope']"),
    ("reference 1-D short", {}, dict(reference=np.zeros(N_GENES - 1, np.float32)), ValueError, REFERENCE),
    ("reference 2-D long", {}, dict(reference=np.zeros((2, N_GENES + 3))), ValueError, REFERENCE),
    ("var_names + mean_order", dict(dup_names=True), dict(mean_order="x"), ValueError, "Ensure your var_names are unique!"),
    ("mean_order + chunksize", {}, dict(mean_order="x", chunksize=0), ValueError, MEAN_ORDER),
    ("chunksize + reference", {}, dict(chunksize=0, reference=np.zeros(3)), ValueError, CHUNKSIZE),
    ("chunksize + complex matrix", dict(dtype=np.complex64), dict(chunksize=-1), ValueError, CHUNKSIZE),
    ("category + complex matrix", dict(dtype=np.complex64), dict(reference_key="group", reference_cat="nope"), ValueError,
     "unsupported matrix dtype complex64"),
    ("reference + complex matrix", dict(dtype=np.complex64), dict(reference=np.zeros(3)), ValueError,
     "unsupported matrix dtype complex64"),
    # a given reference decides: the categories are not looked at
    ("reference + category", {}, dict(reference=np.zeros(3), reference_key="group", reference_cat="nope"), ValueError,
     REFERENCE),
]


@pytest.fixture
def torch_without_device(monkeypatch):
    import torch

    from infercnvpy_amd import _engine

    monkeypatch.setattr(_engine, "_torch", lambda: torch)


@pytest.mark.parametrize("make,kw,exc,msg", [pytest.param(*c[1:], id=c[0]) for c in FAULTS])
def test_host_path_faults(torch_without_device, make, kw, exc, msg):
    import infercnvpy_amd as cnv

    ad = _adata(**make)
    with pytest.raises(exc) as err:
        cnv.tl.infercnv(ad, **kw)
    assert str(err.value) == msg
    assert not ad.obsm and not ad.uns and not ad.layers


@pytest.mark.parametrize("kw,msg", [
    ({}, "infercnv_device: X must be a CUDA torch.Tensor or an infercnvpy_amd.DeviceMatrix "
         "(host matrices go through tl.infercnv)"),
    (dict(chunksize=0, reference=np.zeros(3)), "infercnv_device: X must be a CUDA torch.Tensor or an "
                                               "infercnvpy_amd.DeviceMatrix (host matrices go through tl.infercnv)"),
    (dict(mean_order="x", chunksize=0), MEAN_ORDER),
])
def test_infercnv_device_refuses_a_host_matrix(kw, msg):
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(ValueError) as err:
        cnv.tl.infercnv_device(ad.X, ad.var, ad.obs, **kw)
    assert str(err.value) == msg
    import torch

    with pytest.raises(ValueError) as err:  # a torch tensor in host memory is a host matrix too
        cnv.tl.infercnv_device(torch.from_numpy(ad.X), ad.var, ad.obs, **kw)
    assert str(err.value) == msg

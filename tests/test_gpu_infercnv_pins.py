"""What ``tl.infercnv`` / ``tl.infercnv_device`` do around the numeric work, on a GPU: the arguments the device-resident
path refuses (exception type and whole message), the two warnings (once per call, whatever the number of shards) and the
exact key set of ``_timings`` for one shard, two shards and a resident matrix (``bench.py`` reads these keys).  200 cells on
the small gene layout of test_gpu_multirank.py, ``chunksize=50``."""
import logging

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import cases

pytestmark = pytest.mark.gpu

N_OBS, CHUNK = 200, 50
ALL_CELLS = ("Using mean of all cells as reference. For better results, provide either `reference`, or both "
             "`reference_key` and `reference_cat`. ")
SKIPPED = "Skipped 6 genes because they don't have a genomic position annotated. "
REFERENCE = "Reference must match the number of genes in AnnData. "
CHUNKSIZE = "chunksize must be >= 1"
OWN_DTYPE = ("a device-resident matrix needs a reference of its own (or a narrower) dtype: "
             "numpy would promote the subtraction (pass the matrix as float64)")


@pytest.fixture(scope="module")
def inputs():
    v = cases.synthetic_var([700, 320, 150, 100, 60], extra=(("chrX", 40), ("chrM", 5), (None, 6)))
    X = cases.synthetic_expr(N_OBS, len(v["names"]), seed=77)
    var = pd.DataFrame({"chromosome": v["chromosome"], "start": v["start"], "end": v["end"]}, index=v["names"])
    obs = pd.DataFrame({"group": np.array(["n1", "n2", "t"])[np.random.RandomState(4).randint(0, 3, N_OBS)]})
    ref = X[:50].mean(axis=0, dtype=np.float64).astype(np.float32)
    return X, obs, var, ref


def _run(X, obs, var, **kw):
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    tm = {}
    kw.setdefault("chunksize", CHUNK)
    out = cnv.tl.infercnv(SimpleAnnData(X, obs=obs, var=var), inplace=False, _timings=tm, **kw)
    return out, tm


def _on_gpu(X):
    import torch

    return torch.from_numpy(X).cuda()


def test_resident_path_faults(inputs):
    import infercnvpy_amd as cnv

    X, obs, var, ref = inputs
    Xd = _on_gpu(X)
    n = X.shape[1]

    def both(msg, **kw):
        kw.setdefault("chunksize", CHUNK)
        with pytest.raises(ValueError) as err:
            _run(Xd, obs, var, **kw)
        assert str(err.value) == msg
        with pytest.raises(ValueError) as err:
            cnv.tl.infercnv_device(Xd, var, obs, **kw)
        assert str(err.value) == msg

    both(REFERENCE, reference=ref[:-1])
    both(REFERENCE, reference=np.zeros((2, n + 1), np.float32))
    both(OWN_DTYPE, reference=ref.astype(np.float64))
    both(CHUNKSIZE, chunksize=0, reference=ref)
    both(CHUNKSIZE, chunksize=0, reference=ref[:-1])  # two faults: the chunk size is looked at first
    both(REFERENCE, reference=ref[:-1].astype(np.float64))  # ... and the length before the dtype
    with pytest.raises(ValueError) as err:
        cnv.tl.infercnv_device(Xd, var, None, reference_key="group", reference_cat="n1", chunksize=CHUNK)
    assert str(err.value) == "reference_key needs `obs`"
    with pytest.raises(ValueError) as err:  # (before the chunk size)
        cnv.tl.infercnv_device(Xd, var, None, reference_key="group", reference_cat="n1", chunksize=0)
    assert str(err.value) == "reference_key needs `obs`"
    for bad in (Xd[:, :-1], Xd[:, :100].contiguous()):
        with pytest.raises(ValueError) as err:
            cnv.tl.infercnv_device(bad, var, obs, reference=ref, chunksize=0)
        assert str(err.value) == "X must have one column per row of `var`"
    # obs is not needed where no category is asked for, and the next call works
    pos, x_cnv, gv = cnv.tl.infercnv_device(Xd, var, None, reference=ref, chunksize=CHUNK)
    assert x_cnv.shape[0] == N_OBS and gv is None


def _count(caplog, text):
    return sum(r.getMessage() == text and r.levelno == logging.WARNING for r in caplog.records)


def test_warnings_are_logged_once_per_call(inputs, caplog):
    import infercnvpy_amd as cnv

    X, obs, var, ref = inputs
    calls = [
        (lambda: _run(X, obs, var), 1),
        (lambda: _run(sp.csr_matrix(X), obs, var, devices=[0, 0, 0]), 1),
        (lambda: _run(X, obs, var, mean_order="float64", devices=[0, 0]), 1),
        (lambda: _run(X, obs, var, reference_key="group"), 1),  # (half a request is none)
        (lambda: _run(_on_gpu(X), obs, var), 1),
        (lambda: cnv.tl.infercnv_device(_on_gpu(X), var, chunksize=CHUNK), 1),
        (lambda: _run(X, obs, var, reference=ref, devices=[0, 0, 0]), 0),
        (lambda: _run(X, obs, var, reference_key="group", reference_cat=["n1", "n2"], devices=[0, 0, 0]), 0),
        (lambda: _run(_on_gpu(X), obs, var, reference_key="group", reference_cat="n1"), 0),
    ]
    for call, n_all_cells in calls:
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="infercnvpy_amd"):
            call()
        assert _count(caplog, ALL_CELLS) == n_all_cells
        assert _count(caplog, SKIPPED) == 1
        assert sum(r.name == "infercnvpy_amd" and r.levelno >= logging.WARNING for r in caplog.records) == n_all_cells + 1


BASE = {"devices", "plan", "kernel", "total", "stream_and_kernels", "h2d", "csr_pack_d2h", "csr_pack_d2h_tail",
        "sparse_upload"}
PACK = {"pack_pack_s", "pack_wait_buffer_s", "pack_wait_link_s", "pack_threads"}


def test_timings_keys(inputs):
    import infercnvpy_amd as cnv

    X, obs, var, ref = inputs
    cats = dict(reference_key="group", reference_cat=["n1", "n2"])
    packed = set()
    # (keywords, matrix, means formed)
    for kw, Xin, means in ((dict(reference=ref), X, False), (dict(), X, True), (cats, X, True),
                           (dict(mean_order="float64"), X, True), (dict(reference=ref.astype(np.float64)), X, False),
                           (dict(reference=ref), sp.csr_matrix(X), False), (cats, sp.csr_matrix(X), True),
                           (dict(), sp.csc_matrix(X), True), (dict(), np.asfortranarray(X), True),
                           (dict(reference=ref, calculate_gene_values=True), X, False)):
        _, tm = _run(Xin, obs, var, devices=[0], **kw)
        exp = BASE | ({"reference_pass"} if means else set()) | (PACK if tm["sparse_upload"] else set())
        assert set(tm) == exp, (kw, sorted(set(tm) ^ exp))
        assert tm["devices"] == [0] and isinstance(tm["sparse_upload"], bool)
        packed.add(tm["sparse_upload"])
        _, tm2 = _run(Xin, obs, var, devices=[0, 0], **kw)
        # (what one uploader did -- sparse_upload, pack_* -- is reported per shard only)
        exp2 = (exp - PACK - {"sparse_upload"}) | {"shards", "concat"}
        assert set(tm2) == exp2, (kw, sorted(set(tm2) ^ exp2))
        assert tm2["devices"] == [0, 0] and len(tm2["shards"]) == 2
        whole_columns = sp.issparse(Xin) and Xin.format == "csc" or isinstance(Xin, np.ndarray) and not Xin.flags.c_contiguous
        for k, sh in enumerate(tm2["shards"]):
            exp_sh = (exp - PACK - {"devices", "plan"}) | {"rows", "device"} | (PACK if sh["sparse_upload"] else set())
            if whole_columns:  # formed on the first GPU before the shards start
                exp_sh -= {"reference_pass"}
            assert set(sh) == exp_sh, (kw, k, sorted(set(sh) ^ exp_sh))
            assert sh["rows"] == 100 and sh["device"] == 0
    assert packed == {True, False}  # a float32 matrix of log-counts packs on the host; float64 compute and CSR do not
    for kw in (dict(reference=ref), dict(), cats, dict(reference=ref, calculate_gene_values=True)):
        _, tm = _run(_on_gpu(X), obs, var, **kw)
        assert set(tm) == {"kernel", "devices", "pieces", "total"}
        assert tm["devices"] == [0] and tm["pieces"] == 1
        tm = {}
        cnv.tl.infercnv_device(_on_gpu(X), var, obs, chunksize=CHUNK, _timings=tm, **kw)
        assert set(tm) == {"kernel", "devices", "pieces", "total"}

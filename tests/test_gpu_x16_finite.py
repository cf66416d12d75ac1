"""k_smooth_x16<FINITE>: when it runs, when it must not, and that it changes no bit (``-m gpu``).

Where the library itself formed the reference row as float32 chains over ALL rows it is about to smooth, finite means
prove a finite matrix (a NaN makes its column's chain NaN for good, an infinity makes it infinite or NaN), and the dense
smoothing kernel runs without its per-gene NaN handling.  The host does not wait for the means: it launches both forms
and each reads the finite-means words of ``k_chain_mean`` first.  ``plan.last_kernel()`` reads back which one applied.

Shapes: the small layouts of ``_smooth_cases`` (window 100: the 4096-bin form; ``L250``: the 1024-bin form), ``cu + 1``
and ``2 cu + 1`` rows, so every workgroup runs the fill and the drain of the kernel's pipeline and some run a second cell.
Every comparison is of the same call under the developer knobs ``ICV_NO_X16_FINITE`` (the checked form alone) and
``ICV_FORCE_GENERIC``:

* the two forms of k_smooth_x16 run the same arithmetic in the same order: x_res, medians, thresholds and X_cnv equal;
* against the generic kernel x_res, medians and X_cnv are equal and the thresholds agree to 1e-12, which is what
  ``test_gpu_parity.test_fast_and_generic_kernels_are_bit_identical`` holds between those two kernels (k_smooth_x16 adds
  the chunk moments in another order).
"""
import functools

import numpy as np
import pandas as pd
import pytest

import _smooth_cases as sc
import cases

pytestmark = pytest.mark.gpu

KNOBS = ("ICV_FORCE_GENERIC", "ICV_NO_X16", "ICV_NO_SD", "ICV_NO_X16_FINITE")
MODES = {"finite": (), "checked": ("ICV_NO_X16_FINITE",), "generic": ("ICV_FORCE_GENERIC",)}
CHUNK = 96  # rows per noise-threshold chunk: several chunks, the last one partial
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    from infercnvpy_amd import _lib

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _lib.load().icv_developer_knobs_reload()
    yield
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _lib.load().icv_developer_knobs_reload()


def _set_mode(monkeypatch, mode):
    from infercnvpy_amd import _lib

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k in MODES[mode]:
        monkeypatch.setenv(k, "1")
    _lib.load().icv_developer_knobs_reload()


def _cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows(which):
    return (_cu() + 1, 2 * _cu() + 1)[which]


@functools.lru_cache(maxsize=None)
def _plan(name):
    from infercnvpy_amd._plan import GenePlan

    L = sc.layout(name)
    return GenePlan(L.chromosome, L.start, window_size=L.window, step=L.step)


@functools.lru_cache(maxsize=None)
def _finite_matrix(name, n):
    """Real-valued expression (no NaN, no infinity); shared and left unchanged: the cases that alter it copy it."""
    return cases.synthetic_expr(n, sc.layout(name).G, seed=31)


def _col(L, k=0):
    """A column that takes part in the windows (a gene of the chromosome with 100 windows)."""
    return int(L.cols[L.chrom_of_windows(100)][17 + k])


def _kinds():
    from infercnvpy_amd import _lib

    return {"finite": _lib.ICV_KERNEL_X16_FINITE, "checked": _lib.ICV_KERNEL_X16, "generic": _lib.ICV_KERNEL_GENERIC}


def _call(name, X, monkeypatch, mode, given=None):
    """One call as the resident path of tl.infercnv makes it: means of all rows as chains + the finite-means words (or
    the given profile and no words), smoothing, thresholds, CSR pack.  -> (host arrays, kernel that ran, words)."""
    import torch

    from infercnvpy_amd import _engine

    _set_mode(monkeypatch, mode)
    plan = _plan(name)
    dm = _engine.to_device_matrix(np.ascontiguousarray(X))
    n = X.shape[0]
    words = None
    if given is None:
        acc = _engine.column_chain(dm, None, None, n)
        ref, words = _engine.chain_mean(acc, n, False, finite_words=True)
    else:
        ref = torch.from_numpy(np.ascontiguousarray(given, dtype=np.float32)).cuda()
    res = _engine.run_hot_path(plan, dm, ref, lfc_clip=sc.CLIP, dynamic_threshold=1.5, chunksize=CHUNK, apply=False,
                               finite_words=words)
    packed = _engine.threshold_csr(plan, dm, ref, None, res, lfc_clip=sc.CLIP, chunksize=CHUNK)
    torch.cuda.synchronize()
    kind = plan.last_kernel()
    ip = packed.indptr.cpu().numpy()
    nnz = int(ip[-1])
    got = dict(out=res.out.cpu().numpy(), median=res.cell_median.cpu().numpy(), thr=res.thr.cpu().numpy(), indptr=ip,
               indices=packed.indices[:nnz].cpu().numpy(), data=packed.data[:nnz].cpu().numpy(),
               ref=ref.cpu().numpy())
    return got, kind, None if words is None else words.cpu().numpy()


def _assert_same(a, b, what, thr_tol=None):
    for key in ("out", "median", "indptr", "indices", "data"):
        assert a[key].shape == b[key].shape, (what, key)
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)
    if thr_tol is None:
        assert np.array_equal(a["thr"], b["thr"], equal_nan=True), (what, "thr")
    else:
        np.testing.assert_allclose(a["thr"], b["thr"], rtol=thr_tol, atol=0, equal_nan=True, err_msg=what)


def _three_ways(name, X, monkeypatch, want_default, given=None):
    """The call as it comes, with the checked form forced and on the generic kernel: the kernel ids and equal results.
    ``want_default``: "finite" or "checked", the form the unforced call must take."""
    kinds = _kinds()
    got, kind, words = _call(name, X, monkeypatch, "finite", given)
    chk, kind_c, _ = _call(name, X, monkeypatch, "checked", given)
    gen, kind_g, _ = _call(name, X, monkeypatch, "generic", given)
    print(f"{name} rows {X.shape[0]}: kernels {kind} / {kind_c} / {kind_g}, words {None if words is None else words.tolist()}")
    assert (kind, kind_c, kind_g) == (kinds[want_default], kinds["checked"], kinds["generic"])
    _assert_same(got, chk, "unforced call against the checked x16 kernel")
    _assert_same(got, gen, "unforced call against the generic kernel", thr_tol=1e-12)
    return got, words


LAYOUT_ROWS = [("L100", 0), ("L100", 1), ("L250", 0), ("L250", 1)]


@pytest.mark.parametrize("name,which", LAYOUT_ROWS)
def test_finite_matrix_takes_the_finite_form_and_changes_no_bit(name, which, monkeypatch):
    """(a) a finite matrix, means over all its rows: the FINITE form ran, all words zero, the results those of the
    checked form and of the generic kernel."""
    X = _finite_matrix(name, _rows(which))
    got, words = _three_ways(name, X, monkeypatch, "finite")
    assert words.shape == (16,) and not words.any()
    assert np.isfinite(got["out"]).all() and np.isfinite(got["thr"]).all() and got["indptr"][-1] > 0


@pytest.mark.parametrize("name,which", LAYOUT_ROWS)
@pytest.mark.parametrize("special", ["nan", "inf", "inf_and_minus_inf"])
def test_a_nan_or_an_infinity_keeps_the_checked_form(name, which, special, monkeypatch):
    """(b) one NaN, one +inf, or +inf and -inf in one column: a word is set, the checked form ran, results equal to the
    generic kernel's (NaN rows included)."""
    L = sc.layout(name)
    X = _finite_matrix(name, _rows(which)).copy()
    c = _col(L)
    X[3, c] = np.nan if special == "nan" else np.inf
    if special == "inf_and_minus_inf":
        X[X.shape[0] - 2, c] = -np.inf
    got, words = _three_ways(name, X, monkeypatch, "checked")
    assert words.any() and not np.isfinite(got["ref"][c])
    assert np.isnan(got["out"][3]).any()  # (the row with the special value: NaN - NaN, inf - inf)


@pytest.mark.parametrize("name", ["L100", "L250"])
def test_a_given_reference_proves_nothing(name, monkeypatch):
    """(c) a finite matrix and a profile from the caller: no words are passed, the checked form runs."""
    X = _finite_matrix(name, _rows(0))
    ref = X.mean(axis=0, dtype=np.float64).astype(np.float32)
    _, words = _three_ways(name, X, monkeypatch, "checked", given=ref)
    assert words is None


def _var(L):
    names = [f"g{i}" for i in range(L.G)]
    return pd.DataFrame({"chromosome": L.chromosome, "start": L.start, "end": np.asarray(L.start) + 1}, index=names)


def _public_call(name, X, monkeypatch, mode, **kw):
    """tl.infercnv_device on the resident matrix -> (X_cnv host arrays, kernel id read from the plan the call used)."""
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd.tl import _infercnv as T

    _set_mode(monkeypatch, mode)
    L = sc.layout(name)
    var = _var(L)
    _, res, _ = cnv.tl.infercnv_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(), var, kw.pop("obs", None),
                                       window_size=L.window, step=L.step, chunksize=CHUNK, **kw)
    torch.cuda.synchronize()
    plan = T._cached_plan(var["chromosome"].to_numpy(), var["start"].to_numpy(), L.window, L.step, ("chrX", "chrY"),
                          torch.cuda.current_device())
    m = res.to_scipy()
    return (m.indptr, m.indices, m.data), plan.last_kernel()


@pytest.mark.parametrize("name", ["L100", "L250"])
def test_public_call_passes_the_words_only_for_means_over_all_rows(name, monkeypatch):
    """(a), (c) through the public call on a resident matrix: ``reference=None`` takes the FINITE form; a given
    reference and a ``reference_cat`` whose excluded rows hold a NaN take the checked form.  X_cnv equals the generic
    kernel's every time."""
    kinds = _kinds()
    L = sc.layout(name)
    n = _rows(0)
    X = _finite_matrix(name, n)
    Xn = X.copy()
    Xn[n - 1, _col(L)] = np.nan  # a row outside the reference category
    obs = pd.DataFrame({"grp": ["a"] * (n - 2) + ["b"] * 2}, index=[str(i) for i in range(n)])
    given = X.mean(axis=0, dtype=np.float64).astype(np.float32)
    for what, Xc, kw, want in (("reference=None", X, {}, "finite"),
                               ("given reference", X, dict(reference=given), "checked"),
                               ("reference_cat", Xn, dict(obs=obs, reference_key="grp", reference_cat="a"), "checked")):
        got, kind = _public_call(name, Xc, monkeypatch, "finite", **dict(kw))
        gen, kind_g = _public_call(name, Xc, monkeypatch, "generic", **dict(kw))
        print(f"{name} {what}: kernels {kind} / {kind_g}")
        assert (kind, kind_g) == (kinds[want], kinds["generic"]), what
        for a, b in zip(got, gen):
            assert np.array_equal(a, b, equal_nan=True), what


@pytest.mark.parametrize("name,which", LAYOUT_ROWS)
def test_finite_extremes_take_the_finite_form(name, which, monkeypatch):
    """(d) finite extremes: a value next to the largest float32 against a negative mean, so that ``x - ref`` overflows to
    +inf (the clip gives ``cap``, not NaN), and subnormal values.  The FINITE form ran, results equal to generic.

    (With n >= 257 rows a finite chain bounds the mean by FLT_MAX / n < 1.4e36, so the overflow needs x within that of
    FLT_MAX: 3.4e38 here, and -1.9 FLT_MAX spread over the other rows of the column.)"""
    L = sc.layout(name)
    n = _rows(which)
    X = _finite_matrix(name, n).copy()
    c_big, c_sub = _col(L), _col(L, 1)
    X[:, c_big] = np.float32(-1.9 * FLT_MAX / (n - 1))
    X[2, c_big] = np.float32(3.4e38)
    X[4, c_sub], X[5, c_sub], X[6, c_sub] = np.float32(1e-40), np.float32(-1e-42), np.float32(1.4e-45)
    assert np.isfinite(X).all() and 0 < abs(float(X[4, c_sub])) < float(np.finfo(np.float32).tiny)
    got, words = _three_ways(name, X, monkeypatch, "finite")
    ref = got["ref"]
    assert not words.any() and np.isfinite(ref).all() and ref[c_big] < 0
    with np.errstate(over="ignore"):
        assert np.isposinf(X[2, c_big] - ref[c_big])  # the case is what its name says
    assert np.isfinite(got["out"]).all()


@pytest.mark.parametrize("name", ["L100", "L250"])
def test_the_choice_of_one_call_does_not_survive_into_the_next(name, monkeypatch):
    """(e) two calls in a row on one plan, a NaN matrix then a finite one, and the reverse: each call takes the form its
    own means allow, and the finite matrix gives the same results before and after the NaN call."""
    kinds = _kinds()
    L = sc.layout(name)
    X = _finite_matrix(name, _rows(0))
    Xn = X.copy()
    Xn[3, _col(L)] = np.nan
    first, k1, _ = _call(name, X, monkeypatch, "finite")
    nan1, k2, _ = _call(name, Xn, monkeypatch, "finite")
    again, k3, _ = _call(name, X, monkeypatch, "finite")
    nan2, k4, _ = _call(name, Xn, monkeypatch, "finite")
    print(f"{name}: kernels {k1} {k2} {k3} {k4}")
    assert (k1, k2, k3, k4) == (kinds["finite"], kinds["checked"], kinds["finite"], kinds["checked"])
    _assert_same(again, first, "finite matrix after a NaN matrix")
    _assert_same(nan2, nan1, "NaN matrix after a finite matrix")
    assert np.isnan(nan1["out"]).any() and np.isfinite(again["out"]).all()


@pytest.mark.parametrize("name", ["L100", "L250"])
def test_sharded_path_carries_the_words_of_the_means_over_all_ranks(name, monkeypatch):
    """``dist.reference_means_exact(finite_words=True)`` -> ``dist.run_shard(finite_words=...)`` (one rank): the FINITE
    form ran and X_cnv, medians and thresholds are those of the resident call; without the words the checked form runs."""
    import torch

    from infercnvpy_amd import _engine
    from infercnvpy_amd import dist as icd

    kinds = _kinds()
    X = _finite_matrix(name, _rows(0))
    want, kind, _ = _call(name, X, monkeypatch, "finite")
    plan = _plan(name)
    dm = _engine.to_device_matrix(np.ascontiguousarray(X))
    means, words = icd.reference_means_exact(dm, X.shape[0], finite_words=True)
    got = {}
    for key, fw in (("with", words), ("without", None)):
        res, packed = icd.run_shard(plan, dm, means[0].contiguous(), lfc_clip=sc.CLIP, chunksize=CHUNK, pack=True,
                                    finite_words=fw)
        torch.cuda.synchronize()
        nnz = int(packed.indptr[-1].item())
        got[key] = (plan.last_kernel(), res.cell_median.cpu().numpy(), res.thr.cpu().numpy(),
                    packed.indptr.cpu().numpy(), packed.indices[:nnz].cpu().numpy(), packed.data[:nnz].cpu().numpy())
    print(f"{name}: kernels {kind} / {got['with'][0]} / {got['without'][0]}")
    assert (kind, got["with"][0], got["without"][0]) == (kinds["finite"], kinds["finite"], kinds["checked"])
    assert not words.cpu().numpy().any()
    for g in got.values():
        for a, key in zip(g[1:], ("median", "thr", "indptr", "indices", "data")):
            assert np.array_equal(a, want[key]), key


@pytest.mark.parametrize("name", ["L100", "L250"])
def test_every_instantiation_of_the_finite_form(name, monkeypatch):
    """The FINITE form with per-cell moments (``cell_stats=True``) and with the float64 windows (``windows=True``): the
    same bits as the checked form of the same instantiation."""
    import torch

    from infercnvpy_amd import _engine

    kinds = _kinds()
    X = _finite_matrix(name, _rows(0))
    plan = _plan(name)
    dm = _engine.to_device_matrix(np.ascontiguousarray(X))
    for mode_kw in (dict(cell_stats=True), dict(windows=True)):
        got = {}
        for mode in ("finite", "checked"):
            _set_mode(monkeypatch, mode)
            acc = _engine.column_chain(dm, None, None, X.shape[0])
            ref, words = _engine.chain_mean(acc, X.shape[0], False, finite_words=True)
            res = _engine.run_hot_path(plan, dm, ref, lfc_clip=sc.CLIP, dynamic_threshold=1.5, chunksize=CHUNK,
                                       apply=False, finite_words=words, **mode_kw)
            torch.cuda.synchronize()
            assert plan.last_kernel() == kinds[mode], (mode_kw, mode, plan.last_kernel())
            got[mode] = [t.cpu().numpy() for t in (res.out, res.cell_median, res.thr, res.cell_stats, res.windows)
                         if t is not None]
        assert len(got["finite"]) == 4
        for a, b in zip(got["finite"], got["checked"]):
            assert np.isfinite(a).all() and np.array_equal(a, b), mode_kw


def test_host_path_forms_the_words_from_its_means_pass(monkeypatch):
    """``tl.infercnv`` on a host matrix, ``reference=None``: the means pass over the uploads certifies the matrix, the
    FINITE form runs; with one NaN the checked form; X_cnv equals the generic kernel's both times."""
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    kinds = _kinds()
    L = sc.layout("L100")
    X = _finite_matrix("L100", _rows(0))
    Xn = X.copy()
    Xn[3, _col(L)] = np.nan
    for Xc, want in ((X, "finite"), (Xn, "checked")):
        got = {}
        for mode in ("finite", "generic"):
            _set_mode(monkeypatch, mode)
            tm = {}
            _, res, _ = cnv.tl.infercnv(SimpleAnnData(Xc, var=_var(L)), window_size=L.window, step=L.step, chunksize=CHUNK,
                                        n_jobs=1, inplace=False, _timings=tm)
            got[mode] = (tm["kernel"], res.indptr, res.indices, res.data)
        print(f"host path, {want}: kernels {got['finite'][0]} / {got['generic'][0]}")
        assert (got["finite"][0], got["generic"][0]) == (kinds[want], kinds["generic"])
        for a, b in zip(got["finite"][1:], got["generic"][1:]):
            assert np.array_equal(a, b, equal_nan=True)

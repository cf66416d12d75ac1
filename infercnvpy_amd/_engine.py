"""Device-side execution of the hot path through the C ABI.

PyTorch is used only as plumbing: HBM allocation, H2D/D2H copies and streams.  Every numeric
step runs in ``libinfercnv_hip.so``.  There is no CPU fallback: without a GPU (or without the
built library) the functions here raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time as _time

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._plan import GenePlan


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("infercnvpy_amd needs an AMD GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    return torch


def _stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()


class DeviceMatrix:
    """A cells x genes matrix resident in HBM (dense row-major or CSR), float32 or float64.

    ``DeviceMatrix(dense=tensor)`` or ``DeviceMatrix(indptr=int64, indices=int32, data=float32 / float64,
    shape=(cells, genes))`` (CUDA tensors).  A CSR matrix built by the caller is checked on the device (``validate``,
    one pass over the column indices and one flag read back): row offsets non-decreasing and inside the buffers, column
    indices inside ``[0, genes)``, ascending and unique within every row -- what the host path gets from scipy's
    canonical format.  ``ValueError`` otherwise (unsorted rows would give silently wrong windows)."""

    def __init__(self, *, dense=None, indptr=None, indices=None, data=None, shape=None, indptr_host=None,
                 validate=True):
        torch = _torch()
        if dense is not None:
            if not (isinstance(dense, torch.Tensor) and dense.is_cuda and dense.dim() == 2):
                raise ValueError("DeviceMatrix: `dense` must be a 2-D CUDA tensor")
            if dense.dtype not in (torch.float32, torch.float64):
                raise ValueError("DeviceMatrix: a device matrix must be float32 or float64")
            if dense.stride(1) != 1 and dense.shape[1] > 1:
                raise ValueError("DeviceMatrix: rows must be contiguous (stride 1 along the genes)")
            self.format = _lib.ICV_DENSE
            self.dense = dense
            self.shape = tuple(dense.shape)
            self.dtype = dense.dtype
            self._keep = (dense,)
        else:
            for name, t in (("indptr", indptr), ("indices", indices), ("data", data)):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 1 and t.is_contiguous()):
                    raise ValueError(f"DeviceMatrix: `{name}` must be a contiguous 1-D CUDA tensor")
            if shape is None or len(tuple(shape)) != 2:
                raise ValueError("DeviceMatrix: a CSR matrix needs shape=(cells, genes)")
            if indptr.dtype != torch.int64 or indices.dtype != torch.int32:
                raise ValueError("DeviceMatrix: indptr must be int64 and indices int32")
            if data.dtype not in (torch.float32, torch.float64):
                raise ValueError("DeviceMatrix: a device matrix must be float32 or float64")
            if indptr.numel() != int(shape[0]) + 1:
                raise ValueError("DeviceMatrix: indptr must hold cells + 1 offsets")
            if not (indptr.device == indices.device == data.device):
                raise ValueError("DeviceMatrix: indptr, indices and data must live on one GPU")
            self.format = _lib.ICV_CSR
            self.indptr, self.indices, self.data = indptr, indices, data
            self.shape = (int(shape[0]), int(shape[1]))
            self.dtype = data.dtype
            self._keep = (indptr, indices, data)
            if validate:
                with torch.cuda.device(indptr.device):
                    _lib.check(_lib.load().icv_csr_check(_ptr(indptr), _ptr(indices), self.shape[0], self.shape[1],
                                                         min(indices.numel(), data.numel()), _stream_ptr(torch)))
            # host copy of the row pointers (8 B per row): slices need indptr[row0], indptr[row1]
            self.indptr_host = indptr_host if indptr_host is not None else indptr.cpu().numpy()

    @property
    def device(self):
        return self._keep[0].device

    def row_len_hint(self):
        """CSR: the 99.9 % quantile of the row lengths (computed once from the host copy of the row pointers): what the
        stored-entries kernel sizes its per-cell entry slots with; 0 for dense matrices."""
        if self.format != _lib.ICV_CSR:
            return 0
        hint = getattr(self, "_row_len_hint", None)
        if hint is None:
            lens = np.diff(np.asarray(self.indptr_host))
            hint = int(np.partition(lens, max(0, int(0.999 * (lens.shape[0] - 1))))[max(0, int(0.999 * (lens.shape[0] - 1)))]) \
                if lens.shape[0] else 0
            hint = int(min(max(hint, 0), 2 ** 31 - 1))
            self._row_len_hint = hint
        return hint

    def c_struct(self, row0=0, row1=None):
        """icv_matrix for rows [row0, row1)."""
        torch = _torch()
        n = self.shape[0]
        row1 = n if row1 is None else row1
        m = _lib.Matrix()
        m.format = self.format
        m.dtype = _lib.ICV_F32 if self.dtype == torch.float32 else _lib.ICV_F64
        m.n_rows = row1 - row0
        m.n_cols = self.shape[1]
        esz = 4 if self.dtype == torch.float32 else 8
        if self.format == _lib.ICV_DENSE:
            m.ld = self.dense.stride(0)
            m.values = self.dense.data_ptr() + row0 * self.dense.stride(0) * esz
        else:
            m.ld = 0
            m.values = self.data.data_ptr()
            m.indptr = self.indptr.data_ptr() + 8 * row0  # absolute offsets into indices/values
            m.indices = self.indices.data_ptr()
            m.csr_begin = int(self.indptr_host[row0])
            m.csr_end = int(self.indptr_host[row1])
            m._pad = self.row_len_hint()  # (performance hint of k_smooth_se: the length most rows stay under)
        return m


def to_device_matrix(X, dtype=None, device="cuda"):
    """numpy ndarray / scipy sparse -> DeviceMatrix (host data are copied once)."""
    torch = _torch()
    if isinstance(X, DeviceMatrix):
        return X
    if isinstance(X, torch.Tensor):
        if dtype is not None and X.dtype != dtype:
            X = X.to(dtype)
        return DeviceMatrix(dense=X.to(device).contiguous())
    np_dtype = {None: None, torch.float32: np.float32, torch.float64: np.float64}[dtype]
    if sp.issparse(X):
        X = X.tocsr()
        if not X.has_canonical_format:  # the kernels expect unique, sorted column indices per row
            X = X.copy()
            X.sum_duplicates()
        data = X.data if np_dtype is None else X.data.astype(np_dtype, copy=False)
        indptr64 = X.indptr.astype(np.int64, copy=False)
        return DeviceMatrix(
            validate=False,  # canonical scipy CSR
            indptr_host=indptr64,
            indptr=torch.from_numpy(np.ascontiguousarray(indptr64)).to(device),
            indices=torch.from_numpy(np.ascontiguousarray(X.indices.astype(np.int32, copy=False))).to(device),
            data=torch.from_numpy(np.ascontiguousarray(data)).to(device),
            shape=X.shape,
        )
    if isinstance(X, np.matrix):
        X = np.asarray(X)
    X = np.ascontiguousarray(X if np_dtype is None else X.astype(np_dtype, copy=False))
    return DeviceMatrix(dense=torch.from_numpy(X).to(device))


def column_sums(dm: DeviceMatrix, row_group=None, n_groups=1, sums=None, row0=0, row1=None):
    """float64 per-group column sums of rows [row0, row1), accumulated into ``sums`` (device n_groups x n_cols);
    ``row_group``: group of every one of those rows (-1 = none)."""
    torch = _torch()
    lib = _lib.load()
    if sums is None:
        sums = torch.zeros((n_groups, dm.shape[1]), dtype=torch.float64, device="cuda")
    rg = None
    if row_group is not None:
        rg = torch.as_tensor(np.asarray(row_group, dtype=np.int32)).to("cuda")
    m = dm.c_struct(row0, row1)
    _lib.check(lib.icv_colsum(C.byref(m), _ptr(rg), n_groups, _ptr(sums), _stream_ptr(torch)))
    return sums


def column_chain(dm: DeviceMatrix, acc=None, rows=None, count=None, row0=0, row1=None, cols=None):
    """Continue the reference-order column sums (``icv_colchain``): ``acc`` (device, ``n_cols`` values of the matrix
    dtype; None = start from zero) += the rows ``rows`` (ascending indices RELATIVE to ``row0``; None = all) of
    ``dm[row0:row1]``, added one after the other as numpy's ``np.mean(X, axis=0)`` / scipy's CSR ``mean`` add them.
    ``count``: rows of the WHOLE group (CSR input multiplies every entry by ``1 / count`` first, as scipy does).
    ``cols = (c0, c1)`` (dense only): only the columns [c0, c1) -- ``acc`` stays the full-width vector, its slice is
    continued (the chains of different columns are independent: ranks pipeline over column groups, ``dist.py``)."""
    torch = _torch()
    lib = _lib.load()
    if acc is None:
        acc = torch.zeros(dm.shape[1], dtype=dm.dtype, device="cuda")
    assert acc.dtype == dm.dtype and acc.is_cuda and acc.numel() == dm.shape[1] and acc.is_contiguous()
    m = dm.c_struct(row0, row1)
    acc_ptr = acc.data_ptr()
    if cols is not None:
        c0, c1 = int(cols[0]), int(cols[1])
        if dm.format != _lib.ICV_DENSE:
            raise ValueError("column_chain: column ranges are for dense matrices")
        if not 0 <= c0 <= c1 <= dm.shape[1]:
            raise ValueError("column_chain: column range out of bounds")
        if c1 == c0:
            return acc
        esz = 4 if dm.dtype == torch.float32 else 8
        m.values += c0 * esz
        m.n_cols = c1 - c0
        m._pad = c0  # column offset of the view inside its row (the library's bounds reasoning needs it)
        acc_ptr += c0 * esz
    rows_d, n_sel = None, m.n_rows
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        n_sel = int(rows.shape[0])
        if n_sel == 0:
            return acc
        rows_d = torch.from_numpy(rows).to("cuda")
    scale = 0.0
    if dm.format == _lib.ICV_CSR:
        if not count:
            raise ValueError("column_chain: CSR input needs the row count of the group")
        scale = 1.0 / float(count)
    _lib.check(lib.icv_colchain(C.byref(m), _ptr(rows_d), n_sel, scale, C.c_void_p(acc_ptr), _stream_ptr(torch)))
    return acc


class ChainBlocks:
    """The reference-order float32 chain of a dense float32 matrix BY BLOCKS of rows (``icv_colchain_blocks_*``,
    csrc/icv_kernel_blocks.hpp): what row-sharded ranks run so that they do not take turns on the chain.

        cb = ChainBlocks(dm)                 # workspace on the device
        total = cb.sums()                    # float64 column totals of these rows (concurrent; all-gather them)
        cb.records(est_start)                # block records from the float64 estimate of the chain before row 0
        cb.scan(acc)                         # acc: EXACT float32 chain values before row 0 -> after the last row

    ``scan`` equals ``column_chain(dm, acc)`` bit for bit whatever ``est_start`` was (a wrong estimate costs replays)."""

    def __init__(self, dm: "DeviceMatrix", row0=0, row1=None):
        torch = _torch()
        lib = _lib.load()
        self.dm = dm
        self.m = dm.c_struct(row0, row1)
        nbytes = C.c_int64(0)
        _lib.check(lib.icv_colchain_blocks_workspace(self.m.n_rows, self.m.n_cols, C.byref(nbytes)))
        self.ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device="cuda")
        self.replayed = torch.zeros(1, dtype=torch.int64, device="cuda")

    def sums(self):
        torch = _torch()
        total = torch.empty(self.m.n_cols, dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().icv_colchain_blocks_sums(C.byref(self.m), _ptr(self.ws), _ptr(total), _stream_ptr(torch)))
        return total

    def records(self, est_start=None):
        torch = _torch()
        if est_start is not None:
            assert est_start.dtype == torch.float64 and est_start.is_cuda and est_start.numel() == self.m.n_cols
            est_start = est_start.contiguous()
        _lib.check(_lib.load().icv_colchain_blocks_records(C.byref(self.m), _ptr(self.ws), _ptr(est_start),
                                                           _stream_ptr(torch)))

    def scan(self, acc, cols=None):
        torch = _torch()
        assert acc.dtype == torch.float32 and acc.is_cuda and acc.numel() == self.m.n_cols and acc.is_contiguous()
        c0, c1 = (0, self.m.n_cols) if cols is None else (int(cols[0]), int(cols[1]))
        _lib.check(_lib.load().icv_colchain_blocks_scan(C.byref(self.m), _ptr(self.ws), _ptr(acc), c0, c1,
                                                        _ptr(self.replayed), _stream_ptr(torch)))
        return acc

    def n_blocks(self):
        return (-(-int(self.m.n_rows) // 64)) * int(self.m.n_cols)


def chain_mean(acc, count, is_csr, finite_words=False):
    """Means from the accumulators of :func:`column_chain`: ``acc / count`` in the matrix dtype for dense input
    (numpy's ``true_divide(sum, n)``); CSR accumulators already are the means (scipy scales the entries).

    ``finite_words=True`` (dense only) returns ``(means, words)``: the same kernel also reports, in
    ``_lib.ICV_FINITE_WORDS`` device words, whether every mean it wrote is finite (all zero) -- what
    :func:`run_hot_path` takes as ``finite_words`` where ``acc`` chained ALL rows of the matrix."""
    if is_csr:
        assert not finite_words
        return acc
    torch = _torch()
    lib = _lib.load()
    out = torch.empty_like(acc)
    words = torch.empty(_lib.ICV_FINITE_WORDS, dtype=torch.int32, device="cuda") if finite_words else None
    _lib.check(lib.icv_colchain_mean_finite(_ptr(acc), _lib.ICV_F32 if acc.dtype == torch.float32 else _lib.ICV_F64,
                                            acc.numel(), int(count), _ptr(out), _ptr(words), _stream_ptr(torch)))
    return (out, words) if finite_words else out


def csc_column_means(X, row_group=None, n_groups=1, counts=None, np_dtype=None, max_entries=1 << 28):
    """Per-group column means of a host scipy CSC matrix in scipy's own order (``np.add.reduceat`` per column: first
    stored entry + numpy's pairwise sum of the others, entries scaled by 1 / n first): ``n_groups x n_cols`` host array
    of ``np_dtype``.  The columns travel to the GPU in blocks of at most ``max_entries`` stored entries."""
    torch = _torch()
    lib = _lib.load()
    X = X.tocsc()
    if not X.has_canonical_format:
        X = X.copy()
        X.sum_duplicates()
    np_dtype = np.dtype(np_dtype or (np.float32 if X.dtype == np.float32 else np.float64))
    tdt = torch.float32 if np_dtype == np.float32 else torch.float64
    code = _lib.ICV_F32 if np_dtype == np.float32 else _lib.ICV_F64
    n_cols = X.shape[1]
    indptr = X.indptr.astype(np.int64, copy=False)
    out = np.zeros((n_groups, n_cols), dtype=np_dtype)
    rg = None
    if row_group is not None:
        rg = torch.from_numpy(np.ascontiguousarray(row_group, dtype=np.int32)).cuda()
    if counts is None:
        counts = [X.shape[0]] * n_groups
    c = 0
    while c < n_cols:
        c1 = int(np.searchsorted(indptr, indptr[c] + max_entries, side="right")) - 1
        c1 = min(n_cols, max(c1, c + 1))
        e0, e1 = int(indptr[c]), int(indptr[c1])
        vals = torch.from_numpy(np.ascontiguousarray(X.data[e0:e1].astype(np_dtype, copy=False))).cuda()
        rows = torch.from_numpy(np.ascontiguousarray(X.indices[e0:e1].astype(np.int32, copy=False))).cuda()
        ptr = torch.from_numpy(np.ascontiguousarray(indptr[c:c1 + 1] - e0)).cuda()
        if e1 == e0:  # nothing stored: (the kernel never dereferences empty arrays, but give it valid pointers)
            vals = torch.zeros(1, dtype=tdt, device="cuda")
            rows = torch.zeros(1, dtype=torch.int32, device="cuda")
        for g in range(n_groups):
            mean = torch.empty(c1 - c, dtype=tdt, device="cuda")
            _lib.check(lib.icv_colmean_csc(_ptr(vals), code, _ptr(ptr), _ptr(rows), c1 - c, _ptr(rg), g,
                                           1.0 / float(counts[g]), _ptr(mean), _stream_ptr(torch)))
            out[g, c:c1] = mean.cpu().numpy()
        c = c1
    return out


def fortran_column_means(X, np_dtype=None, max_bytes=1 << 30):
    """All-cell column means of a dense HOST matrix stored column-major (``X.strides[0] < X.strides[1]``: an
    F-ordered array, the transposed view of a genes x cells matrix) in numpy's own order: numpy reduces such a matrix
    column by column with its contiguous inner loop -- pairwise summation over pieces of 8 192 elements -- where a
    C-ordered matrix gets one sequential chain per column (reference tl/_infercnv.py:385).  The columns travel to the GPU
    in blocks as they lie in host memory (``icv_colsum_pairwise``); host array of ``np_dtype``."""
    torch = _torch()
    lib = _lib.load()
    n, g = X.shape
    np_dtype = np.dtype(np_dtype or (np.float32 if X.dtype == np.float32 else np.float64))
    tdt = torch.float32 if np_dtype == np.float32 else torch.float64
    code = _lib.ICV_F32 if np_dtype == np.float32 else _lib.ICV_F64
    XT = X.T
    out = np.empty(g, dtype=np_dtype)
    per = int(max(1, max_bytes // max(1, n * np_dtype.itemsize)))
    for c0 in range(0, g, per):
        c1 = min(g, c0 + per)
        blk = torch.from_numpy(np.ascontiguousarray(XT[c0:c1].astype(np_dtype, copy=False))).cuda()
        sums = torch.empty(c1 - c0, dtype=tdt, device="cuda")
        _lib.check(lib.icv_colsum_pairwise(_ptr(blk), code, n, c1 - c0, n, _ptr(sums), _stream_ptr(torch)))
        out[c0:c1] = chain_mean(sums, n, False).cpu().numpy()
    return out


def free_hbm_bytes():
    """HBM this process can still allocate on the current device: what the driver reports free PLUS the blocks PyTorch's
    caching allocator holds without using them (it hands those out again, or gives them back before it reports out of
    memory) -- after a previous large call the driver's figure alone makes the next call cut its matrix into needless
    slabs (a 1 M-cell matrix was uploaded twice for the reference pass and the smoothing)."""
    torch = _torch()
    free_b, _ = torch.cuda.mem_get_info()
    return int(free_b) + max(0, int(torch.cuda.memory_reserved()) - int(torch.cuda.memory_allocated()))


def alloc_out(rows, n_windows):
    """Device float32 ``rows x n_windows`` result buffer whose rows start on 16-byte boundaries (row stride padded
    to a multiple of 4): the smoothing kernel then writes x_res with 16-byte stores."""
    torch = _torch()
    ld = (n_windows + 3) // 4 * 4
    return torch.empty((rows, ld), dtype=torch.float32, device="cuda")[:, :n_windows]


class SmoothResult:
    windows = None  # float64 windows before centring (run_hot_path(windows=True))

    def __init__(self, out, cell_median, cell_stats, thr, profile):
        self.out = out                  # device float32 C x W (thresholded x_res)
        self.cell_median = cell_median  # device float64 C
        self.cell_stats = cell_stats    # device float64 C x 2 | None (not requested)
        self.thr = thr                  # device float64 n_chunks | None
        self.profile = profile


def _usable_cpus():
    """Logical CPUs this process may really use: the affinity mask, capped by a cgroup CPU quota when one is set."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def _default_pack_threads():
    """Host threads that pack a dense piece (ICV_PACK_THREADS overrides): three quarters of the usable logical CPUs
    (affinity mask and cgroup quota), at most 32.  Measured on the GPU pool's box (2 x 64 cores, but a cgroup quota of 16 CPUs:
    tools/bench_host_pack.py, profiles/r05_host_pack.txt): 124 GB/s of input with 8 threads, 162 with 16, 173 with 32,
    then a collapse (46 GB/s with 64, 20 with 128: the threads are throttled and wait on each other's block tickets)."""
    env = os.environ.get("ICV_PACK_THREADS")
    if env:
        return max(1, int(env))
    # three quarters of the usable CPUs: the packing is bound by host memory, not by the cores (12 threads pack as fast
    # as 16 on a 16-CPU quota: 0.107 / 0.109 s per 16 GB), and the copier, the drain and the page-fault helpers run beside
    # it -- a process that asks for more CPU time than its cgroup grants is stopped for the rest of the 100 ms period
    # (the 0.19 s repeats between 0.14 s ones in profiles/r06_bench_n1.json; 24 / 32 threads: 0.16-0.26 s per call)
    n = _usable_cpus()
    return int(max(1, min(32, n - n // 4)))


# Host buffers of the sparse upload, kept between calls (first-touch page faults of a few GB of fresh pages cost as much as
# the packing itself): at most _PACK_POOL_MAX buffer pairs and _PACK_POOL_BYTES of host memory (six 1 GB pairs
# stayed allocated after the call), handed out largest first; release_pinned_buffers() empties it.
_PACK_POOL = []
_PACK_POOL_LOCK = None
_PACK_POOL_MAX = 6
_PACK_POOL_BYTES = 3 << 30


def _pack_pool_take(np_dtype):
    import threading

    global _PACK_POOL_LOCK
    if _PACK_POOL_LOCK is None:
        _PACK_POOL_LOCK = threading.Lock()
    with _PACK_POOL_LOCK:
        best = None
        for k, b in enumerate(_PACK_POOL):
            if b[1].dtype == np_dtype and (best is None or b[0].shape[0] > _PACK_POOL[best][0].shape[0]):
                best = k
        if best is not None:
            return _PACK_POOL.pop(best)
    return [np.empty(0, np.int32), np.empty(0, np_dtype)]


def _pack_pool_give(bufs):
    if _PACK_POOL_LOCK is None or bufs[0].shape[0] == 0:
        return
    with _PACK_POOL_LOCK:
        held = sum(b[0].nbytes + b[1].nbytes for b in _PACK_POOL)
        if len(_PACK_POOL) < _PACK_POOL_MAX and held + bufs[0].nbytes + bufs[1].nbytes <= _PACK_POOL_BYTES:
            _PACK_POOL.append(bufs)


def _probe_density(X, np_dtype, row0, row1, probe_rows=256):
    """Stored entries per element in ``probe_rows`` rows of X[row0:row1] (a C-ordered float matrix) taken in 16 runs
    spread evenly over the range (a matrix sorted by library size -- empty droplets first -- is not what its
    first rows look like)."""
    n_all = row1 - row0
    n = min(probe_rows, n_all)
    runs = 16 if n_all >= 16 * 16 else 1
    per = max(1, n // runs)
    lib = _lib.load()
    code = _lib.ICV_F32 if np_dtype == np.float32 else _lib.ICV_F64
    total = rows = 0
    for k in range(runs):
        a = row0 + (k * (n_all - per)) // max(runs - 1, 1) if runs > 1 else row0
        xs = X[a:a + per]
        cnt = np.zeros(xs.shape[0], dtype=np.int64)
        _lib.check(lib.icv_host_dense_row_nnz(xs.ctypes.data, code, xs.shape[0], X.shape[1], X.strides[0] // X.itemsize,
                                              cnt.ctypes.data, 1))
        total += int(cnt.sum())
        rows += xs.shape[0]
    return float(total) / float(max(1, rows * X.shape[1]))


def _wants_sparse_upload(X, np_dtype, row0, row1, max_density=0.3):
    """Dense host rows go up as stored entries when they are mostly zeros: a C-ordered float matrix of the compute
    dtype, at least 1024 columns, fewer than ``max_density`` non-zeros in a probe of the first rows.
    ``ICV_NO_SPARSE_UPLOAD`` switches it off (A/B timing)."""
    if os.environ.get("ICV_NO_SPARSE_UPLOAD"):
        return False
    if not isinstance(X, np.ndarray) or X.ndim != 2 or X.dtype != np_dtype or X.shape[1] < 1024 or row1 <= row0:
        return False
    if X.strides[1] != X.itemsize or X.strides[0] < X.shape[1] * X.itemsize or X.strides[0] % X.itemsize:
        return False
    return _probe_density(X, np_dtype, row0, row1) < max_density


class SlabStream:
    """Upload the rows of a host matrix piece by piece on a side stream while the caller computes.

    A helper thread issues the host -> HBM copies (pageable source: the copy call blocks its thread, not the
    caller; measured 56 GB/s on PCIe Gen5 x16, the same as from pinned memory) and records an event per piece;
    ``pieces()`` yields ``(r0, r1)`` in order once the current stream has been made to wait for that piece.
    ``dm`` is the DeviceMatrix of the whole slab (valid row ranges: the pieces yielded so far).
    """

    def __init__(self, X, tdtype, piece_rows, row0=0, row1=None, host_pack_threads=None):
        """Rows [row0, row1) of the host matrix ``X`` (the parent's arrays are read in place: slicing a scipy CSR
        matrix would copy the shard -- 5.6 GB at BASELINE config 4 -- before the first byte is uploaded).
        ``host_pack_threads``: host threads of the sparse upload of a mostly-zero dense matrix (default: the usable
        logical CPUs, at most 32; callers with several shards divide them)."""
        import queue
        import threading

        torch = _torch()
        np_dtype = np.float32 if tdtype == torch.float32 else np.float64
        row1 = X.shape[0] if row1 is None else row1
        self.n_rows = row1 - row0
        self.bounds = [(r, min(self.n_rows, r + piece_rows)) for r in range(0, self.n_rows, piece_rows)]
        self._landed = 0
        device = torch.cuda.current_device()  # the helper threads start on device 0 otherwise
        creator_stream = torch.cuda.current_stream()
        self._err = None
        self._cancel = threading.Event()
        self.sparse_upload = False
        self._packer = None
        # one uploader thread (and stream) per host array: a CSR slab is two arrays, and two threads keep the link
        # busy where one thread alternating between them does not (measured with cold pages and a device -> host
        # copy beside them: 54 against 39 GB/s, tools/exp_h2d_csr.py)
        if sp.issparse(X):
            base = int(X.indptr[row0])  # the slab's entries are [base, base + nnz) of the parent's arrays
            indptr64 = np.ascontiguousarray(X.indptr[row0:row1 + 1].astype(np.int64)) - base
            nnz = int(indptr64[-1])
            d_indices = torch.empty(max(nnz, 1), dtype=torch.int32, device="cuda")
            d_data = torch.empty(max(nnz, 1), dtype=tdtype, device="cuda")
            d_indptr = torch.from_numpy(indptr64).cuda()
            self.dm = DeviceMatrix(indptr=d_indptr, indices=d_indices, data=d_data, shape=(self.n_rows, X.shape[1]),
                                   indptr_host=indptr64, validate=False)  # (filled later, from a canonical matrix)
            idx_h, dat_h = X.indices, X.data

            def copy_indices(r0, r1):
                k0, k1 = int(indptr64[r0]), int(indptr64[r1])
                if k1 > k0:
                    d_indices[k0:k1].copy_(torch.from_numpy(
                        np.ascontiguousarray(idx_h[base + k0:base + k1].astype(np.int32, copy=False))))

            def copy_data(r0, r1):
                k0, k1 = int(indptr64[r0]), int(indptr64[r1])
                if k1 > k0:
                    d_data[k0:k1].copy_(torch.from_numpy(
                        np.ascontiguousarray(dat_h[base + k0:base + k1].astype(np_dtype, copy=False))))

            copiers = [copy_indices, copy_data]
        else:
            dense = torch.empty((self.n_rows, X.shape[1]), dtype=tdtype, device="cuda")
            self.dm = DeviceMatrix(dense=dense)
            self.sparse_upload = _wants_sparse_upload(X, np_dtype, row0, row1)

            def copy_piece(r0, r1):
                dense[r0:r1].copy_(torch.from_numpy(
                    np.ascontiguousarray(X[row0 + r0:row0 + r1].astype(np_dtype, copy=False))))

            if self.sparse_upload:
                # A dense matrix of log-counts is ~80 % zeros and PCIe is what the call waits for: a packer thread turns
                # every piece into (indptr, indices, values) on host threads (icv_host_dense_pack: 8 bytes per stored
                # entry instead of 4 per element), the copier thread sends the three arrays and rebuilds the dense rows
                # in HBM (icv_csr_scatter_dense) -- the slab is bit for bit what the dense copy would have delivered.
                lib = _lib.load()
                code = _lib.ICV_F32 if np_dtype == np.float32 else _lib.ICV_F64
                n_cols = X.shape[1]
                ld = X.strides[0] // X.itemsize
                n_thr = host_pack_threads if host_pack_threads else _default_pack_threads()
                packed_q = queue.Queue(maxsize=2)  # packed pieces waiting for the link
                free_q = queue.Queue()             # recycled host buffers: their pages stay mapped, within the call and
                for _ in range(3):                 # (through the process-wide pool) between calls
                    free_q.put(_pack_pool_take(np_dtype))
                self._pack_bufs = free_q
                self.pack_stats = {"pack_s": 0.0, "wait_buffer_s": 0.0, "wait_link_s": 0.0, "threads": n_thr}
                stats = self.pack_stats
                dens = [max(_probe_density(X, np_dtype, row0, row1), 1e-4)]  # stored entries per element (estimate)

                def pack_all():
                    try:
                        for r0, r1 in self.bounds:
                            if self._cancel.is_set():
                                break
                            xs = X[row0 + r0:row0 + r1]
                            ip = np.empty(r1 - r0 + 1, dtype=np.int64)
                            t1 = _time.perf_counter()
                            bufs = None
                            while bufs is None:  # (a copier that has failed or been cancelled returns nothing)
                                try:
                                    bufs = free_q.get(timeout=0.1)
                                except queue.Empty:
                                    if self._cancel.is_set() or self._err is not None:
                                        return
                            want = int(dens[0] * 1.25 * (r1 - r0) * n_cols) + 4096
                            if bufs[0].shape[0] < want:
                                bufs[0], bufs[1] = np.empty(want, np.int32), np.empty(want, np_dtype)
                            t2 = _time.perf_counter()
                            # one pass over the piece (icv_host_dense_pack_fused); more entries than the buffers hold
                            # (the probe under-estimated the density): grow them and pack again
                            nnz_c = C.c_int64(0)
                            for _ in range(2):
                                rc = lib.icv_host_dense_pack_fused(xs.ctypes.data, code, r1 - r0, n_cols, ld, ip.ctypes.data,
                                                                   bufs[0].ctypes.data, bufs[1].ctypes.data,
                                                                   bufs[0].shape[0], n_thr, C.byref(nnz_c))
                                if rc != _lib.ICV_ERR_NOMEM or nnz_c.value <= bufs[0].shape[0]:
                                    break
                                cap = int(nnz_c.value * 1.1) + 4096
                                bufs[0], bufs[1] = np.empty(cap, np.int32), np.empty(cap, np_dtype)
                                dens[0] = max(dens[0], nnz_c.value / float(max(1, (r1 - r0) * n_cols)))
                            _lib.check(rc)
                            nnz = int(nnz_c.value)
                            t3 = _time.perf_counter()
                            while True:
                                try:
                                    packed_q.put((ip, nnz, bufs), timeout=0.1)
                                    break
                                except queue.Full:
                                    if self._cancel.is_set() or self._err is not None:
                                        return
                            stats["wait_buffer_s"] += t2 - t1
                            stats["pack_s"] += t3 - t2
                            stats["wait_link_s"] += _time.perf_counter() - t3
                    except BaseException as e:  # surfaced by the copier
                        try:
                            packed_q.put(e, timeout=5)
                        except queue.Full:
                            self._err = e

                def copy_piece(r0, r1):  # noqa: F811 -- the sparse form replaces the dense copy
                    # (polled: a packer that was cancelled before it started this piece enqueues nothing -- ADVICE r5)
                    item = None
                    while item is None:
                        try:
                            item = packed_q.get(timeout=0.1)
                        except queue.Empty:
                            if self._err is not None:
                                raise self._err
                            if self._cancel.is_set():
                                raise RuntimeError("sparse upload cancelled")
                            if not self._packer.is_alive() and packed_q.empty():
                                raise RuntimeError("sparse upload: the packer stopped without delivering the piece")
                    if isinstance(item, BaseException):
                        raise item
                    ip, nnz, bufs = item
                    d_ip = torch.from_numpy(ip).cuda()
                    d_idx = torch.empty(max(nnz, 1), dtype=torch.int32, device="cuda")
                    d_val = torch.empty(max(nnz, 1), dtype=tdtype, device="cuda")
                    if nnz:
                        d_idx[:nnz].copy_(torch.from_numpy(bufs[0][:nnz]))
                        d_val[:nnz].copy_(torch.from_numpy(bufs[1][:nnz]))
                    free_q.put(bufs)  # (pageable copies have left the host buffers when copy_ returns)
                    _lib.check(lib.icv_csr_scatter_dense(_ptr(d_val), code, _ptr(d_ip), _ptr(d_idx), r1 - r0, n_cols,
                                                         C.c_void_p(dense[r0:r1].data_ptr()), dense.stride(0),
                                                         _stream_ptr(torch)))

                self._packer = threading.Thread(target=pack_all, daemon=True)

            copiers = [copy_piece]

        self._streams = [torch.cuda.Stream() for _ in copiers]
        self._queues = [queue.Queue() for _ in copiers]
        self._busy = [0.0 for _ in copiers]

        def work(k):
            import time

            t0 = time.perf_counter()
            stream, q, copy = self._streams[k], self._queues[k], copiers[k]
            try:
                torch.cuda.set_device(device)
                # the buffers were allocated on the creator's stream: whatever that stream still has queued on a
                # recycled block (kernels of the previous slab) comes before the first copy into it
                stream.wait_stream(creator_stream)
                with torch.cuda.stream(stream):
                    for r0, r1 in self.bounds:
                        if self._cancel.is_set():
                            break
                        copy(r0, r1)
                        ev = torch.cuda.Event()
                        ev.record(stream)
                        q.put(ev)
                stream.synchronize()
            except BaseException as e:  # surfaced in the consumer
                self._err = e
                q.put(None)
            self._busy[k] = time.perf_counter() - t0

        self._threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(len(copiers))]
        if getattr(self, "_packer", None) is not None:
            self._threads.append(self._packer)
        for th in self._threads:
            th.start()

    @property
    def h2d_seconds(self):
        """Wall-clock seconds the slowest uploader thread took (they run side by side)."""
        return max(self._busy)

    def pieces(self):
        """Row ranges in order; blocks (stream-wise) only for pieces that have not landed yet.  Re-iterable."""
        torch = _torch()
        for k in range(len(self.bounds)):
            if k >= self._landed:
                for q in self._queues:  # a piece has landed when every array's part of it has
                    ev = q.get()
                    if ev is None:
                        raise self._err
                    torch.cuda.current_stream().wait_event(ev)
                self._landed += 1
            yield self.bounds[k]
        self._join()

    def _join(self):
        for th in self._threads:
            if th.is_alive():
                th.join()

    def close(self, cancel=False):
        """Stop the uploader (``cancel``: skip the pieces it has not started) and drop the slab's device buffers."""
        if cancel:
            self._cancel.set()
        self._join()
        bufs_q = getattr(self, "_pack_bufs", None)
        if bufs_q is not None:  # the host buffers of the sparse upload go back to the process-wide pool
            self._pack_bufs = None
            while True:
                try:
                    _pack_pool_give(bufs_q.get_nowait())
                except Exception:
                    break
        if self.dm is not None:
            # kernels of the consumer's stream may still read the slab: the caching allocator must not hand the
            # blocks (allocated on the creator's stream) to anyone before those kernels have run
            torch = _torch()
            cur = torch.cuda.current_stream()
            for t in self.dm._keep:
                t.record_stream(cur)
                for st in self._streams:
                    t.record_stream(st)
        self.dm = None


class PackedRows:
    """x_res of a row range with its keep-mask and per-row counts (device), awaiting the CSR fill."""

    def __init__(self, out, mask, counts, thr):
        self.out, self.mask, self.counts, self.thr = out, mask, counts, thr


def threshold_mask(plan: GenePlan, dm: DeviceMatrix, ref_lo, ref_hi, res, *, lfc_clip, chunksize, row_phase=0,
                   flags=0, row0=0, row1=None):
    """Step 5b without rewriting x_res: keep-bits (|x| >= thr decided in float64, x != 0) + per-row counts."""
    torch = _torch()
    lib = _lib.load()
    rows = res.out.shape[0]
    n_words = (plan.n_windows + 63) // 64
    mask = torch.empty((rows, n_words), dtype=torch.int64, device="cuda")
    counts = torch.empty(rows, dtype=torch.int64, device="cuda")
    m = dm.c_struct(row0, row1)
    _lib.check(lib.icv_threshold_mask(
        plan.handle, C.byref(m), _ptr(ref_lo), _ptr(ref_hi), float(lfc_clip), int(flags), _ptr(res.out),
        res.out.stride(0), _ptr(res.cell_median), _ptr(res.thr), int(chunksize), int(row_phase), _ptr(mask),
        _ptr(counts), _stream_ptr(torch)))
    return PackedRows(res.out, mask, counts, res.thr)


class PackedCsr:
    """X_cnv of a row range as device CSR: ``indptr`` (rows + 1 int64, from 0), ``indices`` (int32) / ``data`` (float64)
    buffers of which the first ``indptr[-1]`` entries are valid.

    This is what ``tl.infercnv`` leaves in ``obsm["X_cnv"]`` for an HBM-resident matrix; ``tl.cnv_score``,
    ``tl.ithcna``, ``tl.cell_linkage`` / ``tl.ward_linkage`` and ``pl.chromosome_heatmap(_summary)`` take it as they
    take the host matrix (the tool functions work on the device arrays; only the plots copy it to the host)."""

    def __init__(self, indptr, indices, data, n_cols, thr=None):
        self.indptr, self.indices, self.data, self.n_cols, self.thr = indptr, indices, data, n_cols, thr

    @property
    def n_rows(self):
        return self.indptr.shape[0] - 1

    @property
    def shape(self):
        return (self.n_rows, self.n_cols)

    @property
    def device(self):
        return self.indptr.device

    def nnz(self):
        """Number of stored entries (reads one value back: synchronises the current stream)."""
        return int(self.indptr[-1].item())

    def to_scipy(self):
        """Host ``scipy.sparse.csr_matrix`` (float64), as the reference returns."""
        ip = self.indptr.cpu().numpy()
        n = int(ip[-1])
        return sp.csr_matrix((self.data[:n].cpu().numpy(), self.indices[:n].cpu().numpy(), ip),
                             shape=(self.n_rows, self.n_cols))

    def toarray(self):
        """Host dense float64 matrix (``scipy``'s ``toarray``)."""
        return self.to_scipy().toarray()

    def dense_rows(self, rows=None):
        """Device float32 ``len(rows) x n_cols`` tile of the selected rows (boolean mask or index array; None = all):
        the input of the fp32 MFMA contractions (``icv_csr_densify``); the values are float32 numbers widened to
        float64, so nothing is rounded.  Row stride padded to 16 bytes."""
        torch = _torch()
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rows_d, n_sel = None, self.n_rows
            if rows is not None:
                rows = np.asarray(rows)
                if rows.dtype == bool:
                    if rows.shape[0] != self.n_rows:
                        raise IndexError("boolean row mask of the wrong length")
                    rows = np.flatnonzero(rows)
                rows = np.ascontiguousarray(rows, dtype=np.int64)
                if rows.size and (rows.min() < 0 or rows.max() >= self.n_rows):
                    raise IndexError("row index out of range")
                n_sel = int(rows.shape[0])
                rows_d = torch.from_numpy(rows).cuda()
            ld = (self.n_cols + 3) // 4 * 4
            out = torch.empty((n_sel, max(ld, 1)), dtype=torch.float32, device="cuda")[:, :self.n_cols]
            code = _lib.ICV_F32 if self.data.dtype == torch.float32 else _lib.ICV_F64
            _lib.check(lib.icv_csr_densify(_ptr(self.data), code, _ptr(self.indptr), _ptr(self.indices), _ptr(rows_d),
                                           n_sel, self.n_cols, _ptr(out), out.stride(0), _stream_ptr(torch)))
        return out


def threshold_csr(plan: GenePlan, dm: DeviceMatrix, ref_lo, ref_hi, res, *, lfc_clip, chunksize, row_phase=0,
                  flags=0, row0=0, row1=None):
    """Step 5b + ``csr_matrix(x_res)`` (reference :449-455) on the device without a host round trip: the un-thresholded
    ``res.out`` of :func:`run_hot_path` (``apply=False``) -> :class:`PackedCsr`.  The entry buffers hold the
    worst case rows x windows; nothing is read back, the call is asynchronous.

    Keep-mask + row counts (``icv_threshold_mask``: ``k_thr_mask_ring``, x_res streamed through an LDS ring),
    ``icv_row_offsets``, ``icv_csr_fill_masked`` (``k_csr_fill_ring``) -- 0.33 ms per 100 000 cells."""
    torch = _torch()
    lib = _lib.load()
    rows = res.out.shape[0]
    W = plan.n_windows
    if (dm.shape[0] if row1 is None else row1) - row0 == 0:  # an empty shard packs to an empty matrix
        return PackedCsr(torch.zeros(1, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
                         torch.empty(1, dtype=torch.float64, device="cuda"), W, res.thr)
    part = threshold_mask(plan, dm, ref_lo, ref_hi, res, lfc_clip=lfc_clip, chunksize=chunksize, row_phase=row_phase,
                          flags=flags, row0=row0, row1=row1)
    cap = rows * W  # (the fill kernels write at the row offsets without a bound: the worst case)
    indptr = torch.empty(rows + 1, dtype=torch.int64, device="cuda")
    indices = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda")
    data = torch.empty(max(cap, 1), dtype=torch.float64, device="cuda")
    st = _stream_ptr(torch)
    _lib.check(lib.icv_row_offsets(_ptr(part.counts), rows, _ptr(indptr), st))
    if rows:
        _lib.check(lib.icv_csr_fill_masked(_ptr(part.out), rows, W, part.out.stride(0), _ptr(part.mask), _ptr(indptr),
                                           _ptr(indices), _ptr(data), st))
    return PackedCsr(indptr, indices, data, W, res.thr)


def concat_packed(parts):
    """Row-wise concatenation of device CSR pieces (reads each piece's entry count back)."""
    torch = _torch()
    ips, idx, dat, thr, off = [parts[0].indptr[:1]], [], [], [], 0
    for p in parts:
        n = p.nnz()
        ips.append(p.indptr[1:] + off)
        idx.append(p.indices[:n])
        dat.append(p.data[:n])
        if p.thr is not None:
            thr.append(p.thr)
        off += n
    return PackedCsr(torch.cat(ips), torch.cat(idx), torch.cat(dat), parts[0].n_cols, torch.cat(thr) if thr else None)


_PAGE = 4096


def _prefault(arrays, start=0, n_threads=8):
    """Write one byte into every page of freshly allocated numpy arrays (from element ``start`` on), from a few
    threads in parallel: numpy releases the GIL for the strided store, the page faults run concurrently."""
    import threading

    jobs = []
    for a in arrays:
        b = a.view(np.uint8).reshape(-1)
        lo = (start * a.itemsize) // _PAGE * _PAGE
        n_pages = (b.shape[0] - lo + _PAGE - 1) // _PAGE
        if n_pages < 256:  # < 1 MB: not worth a thread
            continue
        per = (n_pages + n_threads - 1) // n_threads
        for k in range(n_threads):
            p0, p1 = k * per, min(n_pages, (k + 1) * per)
            if p0 < p1:
                jobs.append(b[lo + p0 * _PAGE: min(b.shape[0], lo + p1 * _PAGE): _PAGE])
    threads = [threading.Thread(target=lambda v=v: v.fill(0)) for v in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()


class _PinnedRing:
    """Device -> pageable host copies through a small ring of pinned staging buffers (one ring per GPU and process).

    A copy straight into pageable memory runs at ~13 GB/s through the driver's staging path and holds back the
    uploads running beside it; here the DMA engine writes 16 MB chunks into pinned slots at link speed and a few
    host threads move them into the final arrays (numpy copies release the GIL)."""

    _rings = {}
    _lock = None

    @classmethod
    def get(cls, torch):
        import atexit
        import threading

        if cls._lock is None:
            cls._lock = threading.Lock()
            atexit.register(cls.release_all)
        dev = torch.cuda.current_device()
        with cls._lock:
            if dev not in cls._rings:
                cls._rings[dev] = cls(torch)
            return cls._rings[dev]

    @classmethod
    def release_all(cls):
        """Drop every GPU's ring (128 MB of pinned host memory and three helper threads each); the next drain builds a
        new one.  Registered with atexit; ``infercnvpy_amd._engine.release_pinned_buffers()`` for long-lived processes."""
        if cls._lock is None:
            return
        with cls._lock:
            rings, cls._rings = cls._rings, {}
        for r in rings.values():
            r.pool.shutdown(wait=True)
            r.slots, r.views = [], []

    def __init__(self, torch, n_slots=8, slot_bytes=16 << 20, n_threads=3):
        import queue
        from concurrent.futures import ThreadPoolExecutor

        self.torch = torch
        self.slot_bytes = slot_bytes
        self.slots = [torch.empty(slot_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(n_slots)]
        self.views = [t.numpy() for t in self.slots]
        self.free = queue.Queue()
        for i in range(n_slots):
            self.free.put(i)
        self.pool = ThreadPoolExecutor(n_threads, thread_name_prefix="icv-d2h")

    def _land(self, i, ev, dst, n):
        try:
            ev.synchronize()
            np.copyto(dst, self.views[i][:n])
        finally:
            self.free.put(i)

    def download(self, src, dst, stream):
        """Enqueue ``dst[...] = src`` (1-D device tensor -> contiguous numpy array of the same dtype and length) on
        ``stream``; returns the futures of the chunks (the copy is complete when all of them are)."""
        torch = self.torch
        src_b = src.view(torch.uint8)
        dst_b = dst.view(np.uint8).reshape(-1)
        n_bytes = src_b.numel()
        assert dst_b.shape[0] == n_bytes
        futs = []
        for a in range(0, n_bytes, self.slot_bytes):
            n = min(self.slot_bytes, n_bytes - a)
            i = self.free.get()
            with torch.cuda.stream(stream):
                self.slots[i][:n].copy_(src_b[a:a + n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
            futs.append(self.pool.submit(self._land, i, ev, dst_b[a:a + n], n))
        return futs


def release_pinned_buffers():
    """Free the pinned staging rings of the device -> host copies (128 MB per GPU used so far, kept between calls) and the
    host buffers of the sparse upload."""
    _PinnedRing.release_all()
    if _PACK_POOL_LOCK is not None:
        with _PACK_POOL_LOCK:
            del _PACK_POOL[:]
    else:
        del _PACK_POOL[:]


class CsrDrain:
    """CSR pack + copy back of finished pieces on a side stream while the caller computes the next ones.

    ``submit(part)`` (a :class:`PackedCsr`: the piece packed on the device by :func:`threshold_csr`; consecutive row
    ranges in order) returns at once, or blocks while ``max_pending`` pieces are still queued (a packed piece holds a
    worst-case buffer).  A helper thread waits for the piece on its own stream, reads the row offsets back and copies
    the packed entries into the final host arrays (sized from the first piece's density, grown if that was too small).
    ``finish()`` returns the scipy CSR matrix of all rows."""

    def __init__(self, n_rows, n_cols, max_pending=2):
        import queue
        import threading

        torch = _torch()
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self._q = queue.Queue()
        self._slots = threading.Semaphore(max_pending)
        self._stream = torch.cuda.Stream()
        self._err = None
        self._cancel = threading.Event()
        self._finished = False
        self.indptr_h = np.zeros(self.n_rows + 1, dtype=np.int64)
        self.indices_h = np.empty(0, dtype=np.int32)
        self.data_h = np.empty(0, dtype=np.float64)
        self.rows_done, self.nnz = 0, 0
        self.busy_seconds = 0.0
        device = torch.cuda.current_device()
        ring = None if os.environ.get("ICV_NO_PINNED_D2H") else _PinnedRing.get(torch)  # knob: A/B timing
        self._pending = []  # futures of chunks on their way into indices_h / data_h
        settle = self._settle

        def reserve(extra, rows_after):
            need = self.nnz + extra
            if need <= self.indices_h.shape[0]:
                return
            settle()  # the arrays are about to be replaced
            # density so far extrapolated to all rows, + 25 %
            est = int(need / max(rows_after, 1) * self.n_rows * 1.25) + 1024 if rows_after < self.n_rows else need
            cap = max(need, est)
            # (plain allocations: huge-page-advised mappings were measured and are 2x slower to fill from the device)
            idx, dat = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.float64)
            # Fresh pages are mapped (and zeroed) by the kernel at first touch.  Left to the device -> host copy, those
            # faults happen inside the driver's copy path, one at a time, and slow the uploads running beside it as
            # well (measured: 39 instead of 55 GB/s host -> HBM).  Touch them here from a few threads instead.
            if not os.environ.get("ICV_NO_PREFAULT"):  # developer knob for A/B timing
                _prefault((idx, dat), start=self.nnz)
            idx[: self.nnz] = self.indices_h[: self.nnz]
            dat[: self.nnz] = self.data_h[: self.nnz]
            self.indices_h, self.data_h = idx, dat

        def work():
            import time

            try:
                torch.cuda.set_device(device)
                with torch.cuda.stream(self._stream):
                    while True:
                        item = self._q.get()
                        if item is None:
                            return
                        if self._cancel.is_set():  # a failed call: drop what is queued, keep draining to the sentinel
                            del item
                            self._slots.release()
                            continue
                        part, ev = item
                        t0 = time.perf_counter()
                        self._stream.wait_event(ev)
                        n = part.n_rows
                        ip, idx_d, dat_d = part.indptr, part.indices, part.data
                        ip_h = ip.cpu().numpy()
                        nnz = int(ip_h[-1])
                        if nnz > idx_d.shape[0]:
                            raise RuntimeError(f"threshold_csr: {nnz} entries for a capacity of {idx_d.shape[0]}")
                        reserve(nnz, self.rows_done + n)
                        if nnz:
                            o = self.nnz
                            if ring is not None:
                                self._pending += ring.download(idx_d[:nnz], self.indices_h[o:o + nnz], self._stream)
                                self._pending += ring.download(dat_d[:nnz], self.data_h[o:o + nnz], self._stream)
                            else:
                                torch.from_numpy(self.indices_h[o:o + nnz]).copy_(idx_d[:nnz])
                                torch.from_numpy(self.data_h[o:o + nnz]).copy_(dat_d[:nnz])
                        # the piece's buffers were allocated on the CONSUMER's stream and are read here on the drain's
                        # (asynchronous copies): the caching allocator must not hand them out before this stream is done
                        # with them
                        for t in (ip, idx_d, dat_d):
                            t.record_stream(self._stream)
                        del idx_d, dat_d
                        self.indptr_h[self.rows_done + 1:self.rows_done + n + 1] = ip_h[1:] + self.nnz
                        self.rows_done += n
                        self.nnz += nnz
                        del part, item, ip
                        self._slots.release()
                        self.busy_seconds += time.perf_counter() - t0
            except BaseException as e:  # surfaced in finish()
                self._err = e
                try:
                    settle()
                except BaseException:
                    pass
                while True:  # keep consuming (and releasing) submitted parts until the sentinel arrives
                    try:
                        if self._q.get(timeout=60) is None:
                            return
                        self._slots.release()
                    except queue.Empty:
                        return

        self._thread = threading.Thread(target=work, daemon=True)
        self._thread.start()

    def _settle(self):
        # (a method, not a closure kept in an attribute: that was a reference cycle, and the drain -- with the host arrays
        # of X_cnv, 3.5 GB at 1 M cells -- stayed alive until the cyclic collector happened to run, inside someone's
        # timed region: profiles/r06_gc_stall.txt)
        pending, self._pending = self._pending, []
        for f in pending:
            f.result()

    def submit(self, part):
        torch = _torch()
        while not self._slots.acquire(timeout=0.05):  # back-pressure: at most max_pending pieces wait for the drain
            if self._err is not None:
                raise self._err
        if self._err is not None:
            raise self._err
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._q.put((part, ev))

    def finish(self, arrays=False):
        """Wait for the queued pieces; the scipy CSR matrix of all rows, or with ``arrays=True`` its
        ``(indptr, indices, data)`` (the caller concatenates several drains)."""
        self._finished = True
        self._q.put(None)
        self._thread.join()
        if self._err is not None:
            raise self._err
        self._settle()
        assert self.rows_done == self.n_rows, (self.rows_done, self.n_rows)
        if arrays:
            return self.indptr_h, self.indices_h[: self.nnz], self.data_h[: self.nnz]
        return sp.csr_matrix((self.data_h[: self.nnz], self.indices_h[: self.nnz], self.indptr_h),
                             shape=(self.n_rows, self.n_cols))

    def close(self):
        """Idempotent shutdown for error paths: drop queued pieces (their device buffers), stop the thread."""
        if not self._finished:
            self._finished = True
            self._cancel.set()
            self._q.put(None)
        if self._thread.is_alive():
            self._thread.join()
        try:
            self._settle()
        except BaseException:
            pass


def run_hot_path(plan: GenePlan, dm: DeviceMatrix, ref_lo, ref_hi=None, *, lfc_clip=3.0, dynamic_threshold=1.5,
                 chunksize=5000, row_phase=0, flags=0, out=None, profile=False, row0=0, row1=None,
                 cell_stats=False, apply=True, windows=False, finite_words=None):
    """Steps 1-5 of the chunk kernel for rows [row0, row1) of ``dm`` (all device-resident).

    ``finite_words``: the words :func:`chain_mean` wrote when it formed ``ref_lo`` from the chains over ALL rows of
    ``dm`` (or of all shards ``dm`` is one of) -- never for a profile from elsewhere or means over a subset of the rows.
    All zero, they certify a finite matrix, and k_smooth_x16 runs without its per-gene NaN handling: the library launches
    both forms and the device picks one (no synchronisation, the same bits).

    ``cell_stats=True`` also returns the per-cell moments (sum, sum of squares of x_res); without them the
    library forms the noise-threshold moments per chunk inside the smoothing kernel (faster).
    ``apply=False`` computes the thresholds but leaves ``out`` un-thresholded (for :func:`threshold_mask`).
    ``windows=True``: the float64 windows before the per-cell centring come back as well (``res.windows``, rows x W:
    what ``calculate_gene_values`` averages, :func:`gene_values_from_windows`) -- written by the same kernel launch."""
    torch = _torch()
    lib = _lib.load()
    n = dm.shape[0]
    row1 = n if row1 is None else row1
    rows = row1 - row0
    W = plan.n_windows
    if out is None:
        out = alloc_out(rows, W)
    assert out.dtype == torch.float32 and out.shape[0] >= rows and out.shape[1] >= W and out.stride(1) == 1
    med = torch.empty(rows, dtype=torch.float64, device="cuda")
    stats = torch.empty((rows, 2), dtype=torch.float64, device="cuda") if cell_stats else None
    if rows == 0:  # a rank that owns no rows (more ranks than chunks): nothing to launch, no chunk, no threshold
        res = SmoothResult(out, med, stats,
                           None if dynamic_threshold is None else torch.empty(0, dtype=torch.float64, device="cuda"), None)
        res.windows = torch.empty((0, W), dtype=torch.float64, device="cuda") if windows else None
        return res
    dyn = float("nan") if dynamic_threshold is None else float(dynamic_threshold)
    thr = None
    if dynamic_threshold is not None:
        n_chunks = max(1, math.ceil((rows + row_phase) / chunksize))
        thr = torch.empty(n_chunks, dtype=torch.float64, device="cuda")
    assert ref_lo.dtype == dm.dtype and ref_lo.is_cuda and ref_lo.numel() == dm.shape[1]
    if ref_hi is not None:
        assert ref_hi.dtype == dm.dtype and ref_hi.is_cuda and ref_hi.numel() == dm.shape[1]
    m = dm.c_struct(row0, row1)
    prof = _lib.Profile() if profile else None
    win = torch.empty((rows, W), dtype=torch.float64, device="cuda") if windows else None
    if finite_words is not None:
        assert finite_words.is_cuda and finite_words.dtype == torch.int32 and finite_words.is_contiguous()
        assert finite_words.numel() == _lib.ICV_FINITE_WORDS and ref_hi is None
    _lib.check(lib.icv_infercnv_run_finite(
        plan.handle, C.byref(m), _ptr(ref_lo), _ptr(ref_hi), float(lfc_clip), dyn, int(chunksize), int(row_phase),
        int(flags) | (0 if apply else _lib.ICV_FLAG_NO_APPLY), _ptr(out), out.stride(0), _ptr(med), _ptr(stats),
        _ptr(thr),
        C.byref(prof) if prof is not None else None, _ptr(win), W, _ptr(finite_words), _stream_ptr(torch)))
    res = SmoothResult(out, med, stats, thr, prof)
    res.windows = win
    return res


def row_abs_sum(x_cnv):
    """per-row sum |x| of a device float32 matrix (cnv_score building block)."""
    torch = _torch()
    lib = _lib.load()
    assert x_cnv.is_cuda and x_cnv.dtype == torch.float32 and x_cnv.stride(1) == 1
    res = torch.empty(x_cnv.shape[0], dtype=torch.float64, device="cuda")
    _lib.check(lib.icv_row_abs_sum(_ptr(x_cnv), x_cnv.shape[0], x_cnv.shape[1], x_cnv.stride(0), _ptr(res),
                                   _stream_ptr(torch)))
    return res


def csr_row_abs_sum(x_csr):
    """per-row sum |x| of a CSR X_cnv (device float64 vector): a host scipy matrix sends only indptr and the stored
    values to the GPU, a :class:`PackedCsr` is read where it lies."""
    torch = _torch()
    lib = _lib.load()
    if isinstance(x_csr, PackedCsr):
        with torch.cuda.device(x_csr.device):
            res = torch.empty(x_csr.n_rows, dtype=torch.float64, device="cuda")
            code = _lib.ICV_F32 if x_csr.data.dtype == torch.float32 else _lib.ICV_F64
            _lib.check(lib.icv_csr_row_abs_sum(_ptr(x_csr.data), code, _ptr(x_csr.indptr), x_csr.n_rows, _ptr(res),
                                               _stream_ptr(torch)))
        return res
    x_csr = x_csr.tocsr()
    data = x_csr.data if x_csr.data.dtype in (np.float32, np.float64) else x_csr.data.astype(np.float64)
    d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    ip = torch.from_numpy(np.ascontiguousarray(x_csr.indptr.astype(np.int64, copy=False))).cuda()
    res = torch.empty(x_csr.shape[0], dtype=torch.float64, device="cuda")
    _lib.check(lib.icv_csr_row_abs_sum(_ptr(d), _lib.ICV_F32 if data.dtype == np.float32 else _lib.ICV_F64, _ptr(ip),
                                       x_csr.shape[0], _ptr(res), _stream_ptr(torch)))
    return res


def group_sums(values, codes, n_groups, want_counts=True):
    """(sums, counts) per group of a device float64 vector: ``codes`` (host int32, -1 = no group) names the group of
    every element.  Fixed summation order on the device (``icv_group_sums``); host numpy arrays of length n_groups
    (``want_counts=False``: counts is None -- one read-back instead of two)."""
    torch = _torch()
    lib = _lib.load()
    with torch.cuda.device(values.device):
        codes_d = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).cuda()
        sums = torch.empty(max(n_groups, 1), dtype=torch.float64, device="cuda")
        counts = torch.empty(max(n_groups, 1), dtype=torch.int64, device="cuda")
        _lib.check(lib.icv_group_sums(_ptr(values), _ptr(codes_d), values.numel(), int(n_groups), _ptr(sums),
                                      _ptr(counts), _stream_ptr(torch)))
        return sums[:n_groups].cpu().numpy(), (counts[:n_groups].cpu().numpy() if want_counts else None)


def gene_values(plan: GenePlan, dm: DeviceMatrix, ref_lo, ref_hi=None, *, lfc_clip=3.0, thr=None, chunksize=5000,
                row_phase=0, flags=0, row0=0, row1=None, out=None):
    """calculate_gene_values for rows [row0, row1): float64 ``rows x n_vars`` device tensor (``out``: written in place),
    NaN where a gene has no value.  ``thr``: the thresholds of the chunks of THOSE rows."""
    torch = _torch()
    lib = _lib.load()
    row1 = dm.shape[0] if row1 is None else row1
    if out is None:
        out = torch.empty((row1 - row0, dm.shape[1]), dtype=torch.float64, device="cuda")
    assert out.dtype == torch.float64 and out.shape[0] == row1 - row0 and out.shape[1] == dm.shape[1]
    assert out.stride(1) == 1 or out.shape[1] <= 1
    m = dm.c_struct(row0, row1)
    _lib.check(lib.icv_gene_values(
        plan.handle, C.byref(m), _ptr(ref_lo), _ptr(ref_hi), float(lfc_clip), int(flags), _ptr(thr), int(chunksize),
        int(row_phase), _ptr(out), out.stride(0), _stream_ptr(torch)))
    return out


def gene_values_from_windows(plan: GenePlan, windows, *, thr=None, chunksize=5000, row_phase=0, n_vars=None, out=None):
    """calculate_gene_values from the float64 windows of :func:`run_hot_path` (``windows=True``): float64
    ``rows x n_vars`` device tensor (``out``: written in place, completely), NaN where a gene has no value.  ONE kernel
    (``icv_gene_values_from_windows``); ``thr``: the thresholds of the chunks of those rows."""
    torch = _torch()
    lib = _lib.load()
    rows = windows.shape[0]
    assert windows.dtype == torch.float64 and windows.is_cuda and (windows.stride(1) == 1 or windows.shape[1] <= 1)
    if out is None:
        out = torch.empty((rows, int(n_vars)), dtype=torch.float64, device="cuda")
    assert out.dtype == torch.float64 and out.shape[0] == rows and (out.stride(1) == 1 or out.shape[1] <= 1)
    _lib.check(lib.icv_gene_values_from_windows(
        plan.handle, _ptr(windows), windows.stride(0), rows, _ptr(thr), int(chunksize), int(row_phase), _ptr(out),
        out.stride(0), _stream_ptr(torch)))
    return out


def corr_iqr(x):
    """IQR of all entries of np.corrcoef(x) for a device float32 matrix (cells x features)."""
    torch = _torch()
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    out = C.c_double()
    _lib.check(lib.icv_corr_iqr(_ptr(x), x.shape[0], x.shape[1], x.stride(0), C.byref(out), _stream_ptr(torch)))
    return float(out.value)


def spare_stride(n):
    """Row stride (floats) of an n x n distance matrix with the n / 2 spare columns the Ward rounds can use."""
    return (n + (n + 1) // 2 + 3) // 4 * 4


def has_spare_columns(dist_sq):
    n = dist_sq.shape[0]
    return dist_sq.stride(0) % 4 == 0 and dist_sq.stride(0) >= n + (n + 1) // 2


def pairwise_sqeuclidean(x, out=None, rows=None, spare=False):
    """float32 squared Euclidean distances between the rows of a device matrix: the full n x n matrix, or the
    row block ``rows = (begin, end)`` against all n rows.  ``spare=True`` (full matrix, no ``out``): allocate the
    result with n / 2 spare columns per row when HBM allows (6 n^2 bytes instead of 4 n^2) -- for a matrix that goes
    on to :func:`ward_linkage` (``spare=has_spare_columns(out)``), whose rounds then write their column updates as
    dense strips."""
    torch = _torch()
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    n = x.shape[0]
    r0, r1 = (0, n) if rows is None else rows
    if out is None:
        ld = (n + 3) // 4 * 4  # a multiple of 16 bytes: vector loads in the Ward rounds
        if rows is None and spare:
            free_b = free_hbm_bytes()
            if 4 * n * spare_stride(n) + 4 * n * (x.shape[1] + 16) + (1 << 30) < free_b:
                ld = spare_stride(n)
        out = torch.empty((r1 - r0, ld), dtype=torch.float32, device=x.device)[:, :n]
    assert out.shape[0] >= r1 - r0 and out.shape[1] >= n and out.stride(1) == 1
    _lib.check(lib.icv_pairwise_sqeuclidean(_ptr(x), n, x.shape[1], x.stride(0), r0, r1, _ptr(out), out.stride(0),
                                            _stream_ptr(torch)))
    return out


def ward_linkage(dist_sq, spare=False):
    """scipy-format Ward linkage matrix from a device n x n squared-distance matrix (overwritten).  ``spare=True``:
    the columns [n, stride) of every row are the rounds' to use as well (a matrix allocated with
    :func:`spare_stride`); False: nothing outside the n x n block is written, whatever the stride."""
    torch = _torch()
    lib = _lib.load()
    assert dist_sq.is_cuda and dist_sq.dtype == torch.float32 and dist_sq.dim() == 2 and dist_sq.stride(1) == 1
    n = dist_sq.shape[0]
    assert dist_sq.shape[1] == n
    Z = np.empty((max(n - 1, 0), 4), dtype=np.float64)
    rounds = C.c_int32(0)
    _lib.check(lib.icv_ward_linkage(_ptr(dist_sq), n, dist_sq.stride(0), 1 if spare else 0, Z.ctypes.data,
                                    C.byref(rounds), _stream_ptr(torch)))
    return Z, int(rounds.value)


def profile_begin(plan: GenePlan):
    """Start deferred timing: later run_hot_path calls on this plan record HIP events without synchronising."""
    _lib.check(_lib.load().icv_profile_begin(plan.handle))


def profile_collect(plan: GenePlan, max_records=4096):
    """End deferred timing; returns the list of _lib.Profile records of the runs since profile_begin."""
    arr = (_lib.Profile * max_records)()
    n = C.c_int32(0)
    _lib.check(_lib.load().icv_profile_collect(plan.handle, arr, max_records, C.byref(n)))
    return [arr[i] for i in range(n.value)]


# ---- tl.pca: X^T X and X V on the device (icv_gram_f64 / icv_project) -------------------------------------------------
class _PcaInput:
    """The matrix tl.pca reads, as DeviceMatrix row slabs: a PackedCsr is read where it lies, a host CSR sends indptr /
    indices / stored values once, a CUDA tensor is used as it is, a host dense array is uploaded slab by slab.
    ``f32_exact``: the stored values are float32 numbers (a float32 Gram panel holds them without rounding)."""

    def __init__(self, x):
        m = matrix_input(x, "tl.pca", slabs=True)
        self.host_dense, self.dm = (m, None) if isinstance(m, np.ndarray) else (None, m)
        # (X_cnv's values are float32 numbers widened to float64)
        self.f32_exact = isinstance(x, PackedCsr) or "float32" in str(m.dtype)
        self.shape = tuple(m.shape)

    def slabs(self, rows):
        """(row0, c_struct) of consecutive slabs of at most `rows` rows."""
        torch = _torch()
        n = self.shape[0]
        for r0 in range(0, n, rows):
            r1 = min(n, r0 + rows)
            if self.dm is not None:
                yield r0, self.dm, self.dm.c_struct(r0, r1)
            else:
                dm = DeviceMatrix(dense=torch.from_numpy(self.host_dense[r0:r1]).cuda())
                yield r0, dm, dm.c_struct()


def _gram_rows(inp, esz_panel, ld):
    """Panel height: a multiple of ICV_GRAM_BLOCK (the Gram's bits do not depend on it) within a quarter of free HBM."""
    blk = _lib.ICV_GRAM_BLOCK
    n = inp.shape[0]
    row_bytes = ld * esz_panel + (inp.shape[1] * inp.host_dense.itemsize if inp.dm is None else 0)
    fit = max(1, int(free_hbm_bytes() // 4 // (row_bytes * blk)))
    return min(fit, max(1, -(-n // blk))) * blk


def gram(x, zero_center=False):
    """(G, colsum): the float64 ``W x W`` Gram matrix X^T X (host numpy, bitwise symmetric) and, when ``zero_center``,
    the float64 column sums (host numpy; None otherwise).  ``x``: PackedCsr, host CSR, host dense or CUDA tensor."""
    torch = _torch()
    lib = _lib.load()
    inp = x if isinstance(x, _PcaInput) else _PcaInput(x)
    n, w = inp.shape
    if n < 1 or w < 1:
        raise ValueError(f"gram: empty matrix of shape {inp.shape}")
    ld = -(-w // 64) * 64
    pdt = torch.float32 if inp.f32_exact else torch.float64
    esz = 4 if inp.f32_exact else 8
    rows = _gram_rows(inp, esz, ld)
    g = torch.empty((w, w), dtype=torch.float64, device="cuda")
    sums = torch.zeros((1, w), dtype=torch.float64, device="cuda") if zero_center else None
    panel = torch.empty((min(rows, -(-n // 32) * 32) * ld,), dtype=pdt, device="cuda")
    code = _lib.ICV_F32 if inp.f32_exact else _lib.ICV_F64
    for r0, dm, m in inp.slabs(rows):
        _lib.check(lib.icv_gram_f64(C.byref(m), code, _ptr(panel), ld, _ptr(g), w, 0 if r0 == 0 else 1,
                                    _stream_ptr(torch)))
        if zero_center:
            column_sums(dm, sums=sums, row0=r0 if inp.dm is not None else 0,
                        row1=(r0 + m.n_rows) if inp.dm is not None else None)
    return g.cpu().numpy(), (sums[0].cpu().numpy() if zero_center else None)


def project(x, V, shift=None, dtype=np.float32):
    """X V - shift (host numpy ``n x k`` of ``dtype``): ``V`` host float64 ``W x k``, ``shift`` host float64 k-vector
    or None; float64 sums in stored-entry order (icv_project)."""
    torch = _torch()
    lib = _lib.load()
    inp = x if isinstance(x, _PcaInput) else _PcaInput(x)
    n, w = inp.shape
    V = np.ascontiguousarray(V, dtype=np.float64)
    k = V.shape[1]
    v_d = torch.from_numpy(V).cuda()
    s_d = torch.from_numpy(np.ascontiguousarray(shift, dtype=np.float64)).cuda() if shift is not None else None
    tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    out = torch.empty((n, k), dtype=tdt, device="cuda")
    rows = n if inp.dm is not None else max(1, int(free_hbm_bytes() // 4 // max(1, w * inp.host_dense.itemsize)))
    for r0, _dm, m in inp.slabs(max(rows, 1)):
        _lib.check(lib.icv_project(C.byref(m), _ptr(v_d), k, _ptr(s_d),
                                   _lib.ICV_F32 if tdt == torch.float32 else _lib.ICV_F64, _ptr(out[r0:]), k,
                                   _stream_ptr(torch)))
    return out.cpu().numpy()


# ---- pp.neighbors: exact kNN and UMAP's fuzzy graph on the device (icv_knn*) -------------------------------------------
def knn(x, n_neighbors, stage_ms=None):
    """(knn_indices, knn_distances, n_exact): the ``n_neighbors - 1`` exact nearest neighbours of every row of the
    device float32 matrix ``x`` (DESIGN.md 4.9 rules 1-3) as device tensors n x (k - 1) (int32, nearest first /
    float32), and the number of rows the certificate sent to the exact kernel.  ``stage_ms``: a list that receives the
    milliseconds of (centring, candidate sweep, re-rank, exact fallback)."""
    torch = _torch()
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and (x.stride(1) == 1 or x.shape[1] <= 1)
    n, d = x.shape
    k = int(n_neighbors)
    need = C.c_int64(0)
    _lib.check(lib.icv_knn_workspace(n, d, k, C.byref(need)))
    with torch.cuda.device(x.device):
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        idx = torch.empty((n, k - 1), dtype=torch.int32, device="cuda")
        dist = torch.empty((n, k - 1), dtype=torch.float32, device="cuda")
        n_exact = C.c_int32(0)
        ms = (C.c_float * 4)() if stage_ms is not None else None
        _lib.check(lib.icv_knn(_ptr(x), n, d, x.stride(0), k, _ptr(ws), _ptr(idx), _ptr(dist), C.byref(n_exact), ms,
                               _stream_ptr(torch)))
    if stage_ms is not None:
        stage_ms[:] = [float(v) for v in ms]
    return idx, dist, int(n_exact.value)


def knn_fuzzy(knn_dist, n_neighbors):
    """(rho, sigma, weights) of rule 5 for the device distances of :func:`knn`: float64 device tensors n, n and
    n x (k - 1)."""
    torch = _torch()
    lib = _lib.load()
    n, km1 = knn_dist.shape
    assert knn_dist.is_cuda and knn_dist.dtype == torch.float32 and knn_dist.is_contiguous() and km1 == n_neighbors - 1
    with torch.cuda.device(knn_dist.device):
        rho = torch.empty(n, dtype=torch.float64, device="cuda")
        sigma = torch.empty(n, dtype=torch.float64, device="cuda")
        w = torch.empty((n, km1), dtype=torch.float64, device="cuda")
        _lib.check(lib.icv_knn_fuzzy(_ptr(knn_dist), n, int(n_neighbors), _ptr(rho), _ptr(sigma), _ptr(w),
                                     _stream_ptr(torch)))
    return rho, sigma, w


def _symmetrize(count_fn, fill_fn, knn_idx, values, k_arg):
    """The canonical CSR (indptr int64, indices int32, data float32; device tensors) that ``count_fn`` / ``fill_fn``
    build from the n x m neighbour table and its float64 values: row lengths, icv_row_offsets, fill."""
    torch = _torch()
    lib = _lib.load()
    n = knn_idx.shape[0]
    assert knn_idx.is_cuda and knn_idx.dtype == torch.int32 and knn_idx.is_contiguous()
    assert values.dtype == torch.float64 and values.is_contiguous() and values.shape == knn_idx.shape
    with torch.cuda.device(knn_idx.device):
        st = _stream_ptr(torch)
        counts = torch.empty(n, dtype=torch.int64, device="cuda")
        _lib.check(count_fn(_ptr(knn_idx), _ptr(values), n, k_arg, _ptr(counts), st))
        indptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        _lib.check(lib.icv_row_offsets(_ptr(counts), n, _ptr(indptr), st))
        nnz = int(indptr[-1].item())
        indices = torch.empty(max(nnz, 1), dtype=torch.int32, device="cuda")
        data = torch.empty(max(nnz, 1), dtype=torch.float32, device="cuda")
        _lib.check(fill_fn(_ptr(knn_idx), _ptr(values), n, k_arg, _ptr(indptr), nnz, _ptr(indices), _ptr(data), st))
    return indptr, indices[:nnz], data[:nnz]


def knn_symmetrize(knn_idx, weights, n_neighbors):
    """C = A + A^T - A o A^T of the membership strengths as canonical CSR, float32, no stored zeros: device tensors
    (indptr int64, indices int32, data float32)."""
    lib = _lib.load()
    k = int(n_neighbors)
    assert knn_idx.shape[1] == k - 1
    return _symmetrize(lib.icv_knn_symmetrize_count, lib.icv_knn_symmetrize_fill, knn_idx, weights, k)


def knn_sorted_rows(knn_idx, knn_dist):
    """The rows of (knn_idx, knn_dist) reordered by ascending column: the indices / data of the distances CSR."""
    torch = _torch()
    lib = _lib.load()
    n, km1 = knn_idx.shape
    with torch.cuda.device(knn_idx.device):
        indptr = torch.arange(n + 1, dtype=torch.int64, device="cuda") * km1
        cols = torch.empty_like(knn_idx)
        vals = torch.empty_like(knn_dist)
        _lib.check(lib.icv_knn_sort_rows(_ptr(indptr), n, _ptr(knn_idx), _ptr(knn_dist), _ptr(cols), _ptr(vals),
                                         _stream_ptr(torch)))
    return indptr, cols.reshape(-1), vals.reshape(-1)


# ---- what tl.leiden, tl.umap and tl.tsne share ---------------------------------------------------------------------------
def _graph_csr(who, indptr, indices, data, dtypes):
    """(indptr, indices, data, n, nnz) of the device CSR graph (indptr int64 n + 1, indices int32, data of one of the
    torch ``dtypes``), contiguous; ValueError for row pointers the kernels could not trust and for 2^31 entries."""
    torch = _torch()
    n = indptr.numel() - 1
    nnz = indices.numel()
    assert indptr.is_cuda and indptr.dtype == torch.int64 and indices.dtype == torch.int32 and data.numel() == nnz
    assert data.dtype in dtypes and n >= 1
    # the kernels trust the row pointers: check them here (two scalars and one comparison on the device)
    if int(indptr[0].item()) != 0 or int(indptr[-1].item()) != nnz or bool((indptr[1:] < indptr[:-1]).any().item()):
        raise ValueError(f"{who}: indptr must start at 0, be non-decreasing and end at the number of stored entries")
    if nnz >= 1 << 31:
        raise ValueError(f"{who}: at most 2^31 - 1 stored entries are supported")
    with torch.cuda.device(indptr.device):
        return indptr.contiguous(), indices.contiguous(), data.contiguous(), n, nnz


def _workspace(fn, *args):
    """The uint8 device tensor (current device) of the size the library's ``fn(*args, &bytes)`` asks for."""
    need = C.c_int64(0)
    _lib.check(fn(*args, C.byref(need)))
    return _torch().empty(need.value, dtype=_torch().uint8, device="cuda")


def _add_stage_ms(stage_ms, names, ms):
    """Add the milliseconds ``ms`` of the stages ``names`` to what the dict ``stage_ms`` holds (None: nothing)."""
    if stage_ms is not None:
        for name, v in zip(names, ms):
            stage_ms[name] = stage_ms.get(name, 0.0) + float(v)


# ---- tl.leiden: Leiden on the device (icv_leiden*) --------------------------------------------------------
LEIDEN_MAX_ITERATIONS = 64


def leiden_quality(e, K, resolution):
    """Q of rule 3 from the communities' integer sums (math.fsum: exactly rounded, independent of the order)."""
    M = sum(K)
    if M == 0:
        return 0.0
    Mf = float(M)
    return math.fsum((float(ec) - resolution * float(kc) * float(kc) / Mf) / Mf for ec, kc in zip(e, K))


def leiden_quantise(indptr, indices, data, use_weights=True):
    """Rules 1-2 of DESIGN.md 4.10 (icv_leiden_quantise) for the device CSR graph (indptr int64 n + 1, indices int32,
    data float32 / float64): (q_indptr int64 n + 1, q_indices int32, q_weights int64, total) with the kept entries only
    and total = the sum of the integer weights; ValueError for every violation of rule 1 or 2."""
    torch = _torch()
    lib = _lib.load()
    indptr, indices, data, n, nnz = _graph_csr("tl.leiden", indptr, indices, data, (torch.float32, torch.float64))
    with torch.cuda.device(indptr.device):
        q_indptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        q_indices = torch.empty(max(nnz, 1), dtype=torch.int32, device="cuda")
        q_w = torch.empty(max(nnz, 1), dtype=torch.int64, device="cuda")
        res = (C.c_int64 * 2)()
        _lib.check(lib.icv_leiden_quantise(_ptr(indptr), _ptr(indices), _ptr(data),
                                           _lib.ICV_F32 if data.dtype == torch.float32 else _lib.ICV_F64, n, nnz,
                                           int(bool(use_weights)), _ptr(q_indptr), _ptr(q_indices), _ptr(q_w), res,
                                           _stream_ptr(torch)))
    kept = int(res[0])
    return q_indptr, q_indices[:kept], q_w[:kept], int(res[1])


def leiden_workspace(n, nnz):
    """The uint8 device tensor leiden_iteration needs for a graph of n vertices and nnz integer entries."""
    return _workspace(_lib.load().icv_leiden_workspace, n, nnz)


def leiden_iteration(q_indptr, q_indices, q_w, gom, seed, it, labels, workspace, stage_ms=None):
    """ONE iteration of rule 4 (icv_leiden_iteration) of the integer graph of leiden_quantise from the partition in
    ``labels`` (device int32 n, ids in [0, n); overwritten by the new partition, not renumbered): (vertices per level,
    (local moving, refinement) rounds per level, local moves of all levels, whether a rule-5 bound was reached).
    ``gom`` = resolution / float(total), ``seed`` in [0, 2^64), ``it`` the iteration's index, ``workspace`` of
    leiden_workspace(n, entries); ``stage_ms``: a ctypes float[4] that receives the stage times."""
    torch = _torch()
    lib = _lib.load()
    n = q_indptr.numel() - 1
    nnz = q_indices.numel()
    assert q_indptr.is_cuda and q_indptr.dtype == torch.int64 and q_indices.dtype == torch.int32
    assert q_w.dtype == torch.int64 and q_w.numel() == nnz and q_indices.is_contiguous() and q_w.is_contiguous()
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.numel() == n and labels.is_contiguous()
    trace = (C.c_int32 * (3 * 64))()
    n_levels, n_moves, bound = C.c_int32(0), C.c_int64(0), C.c_int32(0)
    with torch.cuda.device(q_indptr.device):
        _lib.check(lib.icv_leiden_iteration(_ptr(q_indptr), _ptr(q_indices), _ptr(q_w), n, nnz, float(gom), int(seed),
                                            int(it), _ptr(labels), _ptr(workspace), trace, C.byref(n_levels),
                                            C.byref(n_moves), C.byref(bound), stage_ms, _stream_ptr(torch)))
    nl = n_levels.value
    return ([int(trace[3 * i]) for i in range(nl)], [(int(trace[3 * i + 1]), int(trace[3 * i + 2])) for i in range(nl)],
            int(n_moves.value), bool(bound.value))


def leiden(indptr, indices, data, resolution=1.0, random_state=0, n_iterations=-1, use_weights=True, stages=None):
    """(labels, info) of DESIGN.md 4.10 for the device CSR graph (indptr int64 n + 1, indices int32, data float32 /
    float64; rows sorted): labels is a device int32 tensor numbered by rule 6.  ``stages``: a list that receives one
    dict of milliseconds per iteration."""
    torch = _torch()
    lib = _lib.load()
    n = indptr.numel() - 1
    seed = int(random_state) & ((1 << 64) - 1)
    info = {"quality": [], "n_iterations": 0, "levels": [], "rounds": [], "bound_reached": False}
    t0 = _time.perf_counter()
    q_indptr, q_indices, q_w, M = leiden_quantise(indptr, indices, data, use_weights)
    quantise_ms = (_time.perf_counter() - t0) * 1e3
    with torch.cuda.device(indptr.device):
        st = _stream_ptr(torch)
        labels = torch.arange(n, dtype=torch.int32, device="cuda")
        out = labels  # without weight: n singletons, numbered by rule 6 already
        n_comm = C.c_int32(n)
        if M > 0:
            gom = float(resolution) / float(M)
            ws = leiden_workspace(n, q_indices.numel())
            out = torch.empty_like(labels)
            info["workspace_bytes"] = int(ws.numel())
            e = torch.empty(n, dtype=torch.int64, device="cuda")
            K = torch.empty(n, dtype=torch.int64, device="cuda")
            ms = (C.c_float * 4)() if stages is not None else None
            it = 0
            while True:
                if n_iterations > 0 and it == n_iterations:
                    break
                if it == LEIDEN_MAX_ITERATIONS:
                    info["bound_reached"] = info["bound_reached"] or n_iterations < 0
                    break
                levels, rounds, moves, bound = leiden_iteration(q_indptr, q_indices, q_w, gom, seed, it, labels, ws, ms)
                it += 1
                info["levels"].append(levels)
                info["rounds"].append(rounds)
                info["bound_reached"] = info["bound_reached"] or bound
                _lib.check(lib.icv_leiden_renumber(_ptr(labels), n, _ptr(out), C.byref(n_comm), st))
                _lib.check(lib.icv_leiden_sums(_ptr(q_indptr), _ptr(q_indices), _ptr(q_w), n, _ptr(out), _ptr(e), _ptr(K),
                                               st))
                c = n_comm.value
                info["quality"].append(leiden_quality(e[:c].tolist(), K[:c].tolist(), float(resolution)))
                if stages is not None:
                    stages.append({"local_moving_ms": float(ms[0]), "refinement_ms": float(ms[1]),
                                   "aggregation_ms": float(ms[2]), "rest_ms": float(ms[3]), "quantise_ms": quantise_ms})
                if n_iterations < 0 and moves == 0:
                    break
            info["n_iterations"] = it
        info["n_communities"] = int(n_comm.value)
    return out, info


# ---- tl.umap: the layout epochs on the device (icv_umap*) --------------------------------------------------
def umap_epochs(indptr, indices, data, y, *, a, b, gamma=1.0, negative_sample_rate=5, initial_alpha=1.0, n_epochs,
                epoch_begin=0, epoch_end=None, random_state=0, stage_ms=None):
    """Run the epochs [epoch_begin, epoch_end) of an n_epochs schedule of DESIGN.md 4.11 on the positions ``y`` (device
    float32 n x c, c in (2, 3), contiguous; updated in place and returned) for the device CSR graph (indptr int64
    n + 1, indices int32, data float32; rows sorted, symmetric).  ``stage_ms``: a dict that receives the milliseconds
    of the validation and of the epochs (added to what it holds)."""
    torch = _torch()
    lib = _lib.load()
    assert y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and y.dim() == 2
    assert y.shape[0] == indptr.numel() - 1
    indptr, indices, data, n, nnz = _graph_csr("tl.umap", indptr, indices, data, (torch.float32,))
    c = int(y.shape[1])
    epoch_end = n_epochs if epoch_end is None else epoch_end
    seed = int(random_state) & ((1 << 64) - 1)
    with torch.cuda.device(indptr.device):
        st = _stream_ptr(torch)
        ws = _workspace(lib.icv_umap_workspace, n, nnz, c)
        ms = (C.c_float * 2)() if stage_ms is not None else None
        _lib.check(lib.icv_umap_epochs(_ptr(indptr), _ptr(indices), _ptr(data), n, nnz, c, float(a), float(b),
                                       float(gamma), int(negative_sample_rate), float(initial_alpha), int(n_epochs),
                                       int(epoch_begin), int(epoch_end), seed, _ptr(y), _ptr(ws), ms, st))
        _add_stage_ms(stage_ms, ("validation_ms", "epochs_ms"), ms)
    return y


# ---- tl.tsne: affinities and gradient iterations on the device (icv_tsne*) ---------------------------------
def tsne_affinities(knn_dist, perplexity):
    """(beta, cond) of rule 2 for the device distances of :func:`knn` (n x kk float32, nearest first): float64 device
    tensors n and n x kk."""
    torch = _torch()
    lib = _lib.load()
    n, kk = knn_dist.shape
    assert knn_dist.is_cuda and knn_dist.dtype == torch.float32 and knn_dist.is_contiguous()
    with torch.cuda.device(knn_dist.device):
        beta = torch.empty(n, dtype=torch.float64, device="cuda")
        cond = torch.empty((n, kk), dtype=torch.float64, device="cuda")
        _lib.check(lib.icv_tsne_affinities(_ptr(knn_dist), n, kk, float(perplexity), _ptr(beta), _ptr(cond),
                                           _stream_ptr(torch)))
    return beta, cond


def tsne_symmetrize(knn_idx, cond):
    """W = A + A^T of the conditional affinities as canonical CSR, float32, no stored zeros: device tensors (indptr int64,
    indices int32, data float32)."""
    lib = _lib.load()
    return _symmetrize(lib.icv_tsne_symmetrize_count, lib.icv_tsne_symmetrize_fill, knn_idx, cond, int(knn_idx.shape[1]))


def tsne_iterations(indptr, indices, data, y, update, gains, *, early_exaggeration=12.0, exaggeration_iters=250,
                    learning_rate=1000.0, iter_begin=0, iter_end, stage_ms=None):
    """Run the iterations [iter_begin, iter_end) of DESIGN.md 4.12 on the state (``y``, ``update``, ``gains``: device
    float32 n x c, c in (2, 3), contiguous; updated in place and returned) for the device CSR graph W (indptr int64
    n + 1, indices int32, data float32; rows sorted, symmetric).  ``stage_ms``: a dict that receives the milliseconds
    of the validation and of the iterations (added to what it holds)."""
    torch = _torch()
    lib = _lib.load()
    for s in (y, update, gains):
        assert s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and s.dim() == 2 and s.shape == y.shape
    assert y.shape[0] == indptr.numel() - 1
    indptr, indices, data, n, nnz = _graph_csr("tl.tsne", indptr, indices, data, (torch.float32,))
    c = int(y.shape[1])
    with torch.cuda.device(indptr.device):
        st = _stream_ptr(torch)
        ws = _workspace(lib.icv_tsne_workspace, n, nnz, c)
        ms = (C.c_float * 2)() if stage_ms is not None else None
        _lib.check(lib.icv_tsne_iterations(_ptr(indptr), _ptr(indices), _ptr(data), n, nnz, c, float(early_exaggeration),
                                           int(exaggeration_iters), float(learning_rate), int(iter_begin), int(iter_end),
                                           _ptr(y), _ptr(update), _ptr(gains), _ptr(ws), ms, st))
        _add_stage_ms(stage_ms, ("validation_ms", "iterations_ms"), ms)
    return y, update, gains


# ---- tl.cnv_states: sums of squares and the per-chromosome Viterbi chains on the device (icv_states_*) -------------------
def _empty(torch, n, dtype):
    """An uninitialised CUDA vector of n elements (n may be 0: no allocation of no bytes)."""
    return torch.empty(max(n, 1), dtype=dtype, device="cuda")[:n]


def matrix_input(x, who, slabs=False):
    """The matrix of ``obsm["X_cnv"]`` as one DeviceMatrix: a PackedCsr is read where it lies, a host CSR / CSC sends
    indptr / indices / stored values once (canonical CSR: ascending unique columns), a CUDA tensor is used as it is, a
    host dense array is uploaded.  Values stay float32 or float64; any other dtype becomes float64.  ``who`` prefixes the
    messages.  ``slabs``: the caller slices rows (tl.pca): a host dense array comes back as a contiguous host array, to
    be uploaded slab by slab, and the row pointers of a PackedCsr are copied to the host; without it nothing is read
    back."""
    torch = _torch()
    if isinstance(x, PackedCsr):
        ip = x.indptr.cpu().numpy() if slabs else np.zeros(x.n_rows + 1, dtype=np.int64)
        return DeviceMatrix(indptr=x.indptr, indices=x.indices, data=x.data, shape=x.shape, indptr_host=ip,
                            validate=False)
    if isinstance(x, torch.Tensor):
        if x.dim() != 2:
            raise ValueError(f"{who}: X must be 2-D")
        t = x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float64)
        return DeviceMatrix(dense=t.cuda().contiguous())
    if sp.issparse(x):
        x = x.tocsr()
        if x.data.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        return to_device_matrix(x)
    a = np.asarray(x)
    if a.ndim != 2:
        raise ValueError(f"{who}: X must be 2-D")
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return np.ascontiguousarray(a) if slabs else to_device_matrix(a)


def _chr_start_upload(torch, chr_start):
    """(CUDA int32 copy, C) of ``chr_start``, the host array of C + 1 ascending window numbers from 0 to W; on the
    current device."""
    chr_start = np.ascontiguousarray(chr_start, dtype=np.int32)
    return torch.from_numpy(chr_start).cuda(), int(chr_start.shape[0]) - 1


def _group_lists_upload(torch, rows, group_ptr):
    """(rows, group_ptr, G) as CUDA int64 tensors: host arrays are uploaded to the current device, CUDA tensors are used
    as they are."""
    d_rows, d_ptr = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).cuda()
                     for v in (rows, group_ptr))
    assert d_rows.dtype == torch.int64 and d_ptr.dtype == torch.int64 and d_rows.is_cuda and d_ptr.is_cuda
    assert d_ptr.shape[0] >= 1
    return d_rows, d_ptr, int(d_ptr.shape[0]) - 1


def states_rowsq(dm: DeviceMatrix):
    """(q, nonfinite): the device float64 vector of the per-row sums of v v over the stored entries in stored order
    (DESIGN.md 4.13 rule 1) and a device int32 flag that is 1 when a value is not finite.  No synchronisation."""
    torch = _torch()
    lib = _lib.load()
    with torch.cuda.device(dm.device):
        q = _empty(torch, dm.shape[0], torch.float64)
        flag = torch.empty(1, dtype=torch.int32, device="cuda")
        m = dm.c_struct()
        _lib.check(lib.icv_states_rowsq(C.byref(m), _ptr(q), _ptr(flag), _stream_ptr(torch)))
    return q, flag


def states_absmax(values):
    """Device float64 tensor of one element: the largest ``|v|`` of a CUDA tensor of values (0.0 for an empty one, NaN
    where one is NaN), the ``m`` of DESIGN.md 4.13 rule 6.  Two reductions that allocate nothing of the tensor's size;
    nothing is read back."""
    torch = _torch()
    with torch.cuda.device(values.device):
        if values.numel() == 0:
            return torch.zeros(1, dtype=torch.float64, device="cuda")
        lo, hi = torch.aminmax(values)
        return torch.maximum(-lo, hi).to(torch.float64).reshape(1)


def states_stored_values(dm: DeviceMatrix):
    """The CUDA tensor that holds the stored values of ``dm``: the dense matrix, or the whole data buffer of a CSR one."""
    return dm.dense if dm.format == _lib.ICV_DENSE else dm.data


def flag_and_absmax(flag, absmax):
    """(flag word as an int, largest |v| as a float) of :func:`states_rowsq` or :func:`group_profiles` and
    :func:`states_absmax`: the two device scalars in one copy to the host (the one synchronisation the flag needs anyway)."""
    torch = _torch()
    both = torch.cat([flag.to(torch.float64).reshape(1), absmax]).cpu().tolist()
    return int(both[0]), float(both[1])


def _hmm_call(entry, dm: DeviceMatrix, chr_start, scalars, outputs):
    """The call shape of the three chain kernels: ``chr_start`` (host int32 array of C + 1 ascending window numbers from 0
    to W) is uploaded, ``outputs(torch)`` allocates the tuple of result tensors (None for one that is not wanted) on
    ``dm``'s device, and ``entry(matrix, chr_start, C, *scalars, *outputs, stream)`` is enqueued on the current stream
    (a scalar that is an int or a ctypes array is passed as it is, every other as a float).  Returns the outputs; nothing
    is read back."""
    torch = _torch()
    with torch.cuda.device(dm.device):
        cs, n_chr = _chr_start_upload(torch, chr_start)
        out = outputs(torch)
        m = dm.c_struct()
        _lib.check(entry(C.byref(m), _ptr(cs), n_chr, *(v if isinstance(v, (int, C.Array)) else float(v) for v in scalars),
                         *(_ptr(t) for t in out), _stream_ptr(torch)))
    return out


def states_viterbi(dm: DeviceMatrix, chr_start, *, amplitude, h, stay, sw):
    """(states, nonneutral): device int8 ``n x W`` of -1 / 0 / +1 and device int32 counts of the windows that are not 0
    (DESIGN.md 4.13 rules 2-5).  ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W.  The
    launch is enqueued on the current stream; nothing is read back."""
    n, w = dm.shape
    return _hmm_call(_lib.load().icv_states_viterbi, dm, chr_start, (amplitude, h, stay, sw), lambda torch: (
        torch.empty((n, w), dtype=torch.int8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")))


def _levels_arg(levels, neutral):
    """(the K state means as a ctypes array, K, neutral): what the three icv_copy_* chain entries take for the model's
    levels.  ``levels``: host floats, ``levels[neutral] == 0``."""
    k = len(levels)
    return (C.c_double * k)(*(float(v) for v in levels)), k, int(neutral)


def copy_states_viterbi(dm: DeviceMatrix, chr_start, *, levels, neutral, h, stay, sw):
    """(states, sign, nonneutral): device int8 ``n x W`` of ``state - neutral``, the same clipped to -1 / 0 / +1, and
    device int32 counts of the windows that are not 0 (DESIGN.md 4.22 rules 2-5).  ``levels``: the K state means (host
    floats, ``levels[neutral] == 0``); ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W.  The
    launch is enqueued on the current stream; nothing is read back."""
    n, w = dm.shape
    return _hmm_call(_lib.load().icv_copy_states_viterbi, dm, chr_start, (*_levels_arg(levels, neutral), h, stay, sw),
                     lambda torch: (torch.empty((n, w), dtype=torch.int8, device="cuda"),
                                    torch.empty((n, w), dtype=torch.int8, device="cuda"),
                                    torch.empty(n, dtype=torch.int32, device="cuda")))


def states_fraction(count, n_windows):
    """Device float64 vector ``count / n_windows`` of the device int32 counts of :func:`states_viterbi`: the correctly
    rounded quotient (``icv_states_fraction``), the bits the host's division gives.  Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    with torch.cuda.device(count.device):
        out = torch.empty(count.shape[0], dtype=torch.float64, device="cuda")
        _lib.check(lib.icv_states_fraction(_ptr(count), count.shape[0], int(n_windows), _ptr(out), _stream_ptr(torch)))
    return out


def changepoint_levels(dm: DeviceMatrix, chr_start, *, beta, min_windows):
    """(levels, starts, n_segments): device float64 ``n x W`` level of every window's segment, device uint8 ``n x W`` with 1
    at the first window of every segment, and their integer row sums as device int32 (DESIGN.md 4.19 rules 1-5).
    ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W, no chromosome above
    ``ICV_CHANGEPOINT_MAX_CHR_WINDOWS``.  Enqueued on the current stream; no result is read back."""
    n, w = dm.shape
    levels, starts = _hmm_call(_lib.load().icv_changepoint_levels, dm, chr_start, (beta, int(min_windows)), lambda torch: (
        torch.empty((n, w), dtype=torch.float64, device="cuda"), torch.empty((n, w), dtype=torch.uint8, device="cuda")))
    return levels, starts, starts.sum(dim=1, dtype=_torch().int32)


def changepoint_diffsq(dm: DeviceMatrix, chr_start):
    """Device float64 vector of the ``d_r`` of DESIGN.md 4.19 rule 6: per row the sum over the chromosomes, in ascending
    order, of each chromosome's chain of squared differences of adjacent windows.  No result is read back."""
    return _hmm_call(_lib.load().icv_changepoint_diffsq, dm, chr_start, (), lambda torch: (
        _empty(torch, dm.shape[0], torch.float64),))[0]


# ---- tl.cnv_posteriors / tl.cnv_states_filter: forward-backward chains and the posterior filter --------
def posterior_chains(dm: DeviceMatrix, chr_start, *, amplitude, h, ps, pw, all_states=False):
    """(neutral, loss, gain): device float64 ``n x W`` posteriors of DESIGN.md 4.15 rules 2-5; ``loss`` and ``gain`` are
    None unless ``all_states``.  ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W.  The
    launch is enqueued on the current stream; nothing is read back."""
    shape, wanted = tuple(dm.shape), (True, all_states, all_states)
    return _hmm_call(_lib.load().icv_posterior_chains, dm, chr_start, (amplitude, h, ps, pw), lambda torch: tuple(
        torch.empty(shape, dtype=torch.float64, device="cuda") if k else None for k in wanted))


def posterior_stats(dm: DeviceMatrix, chr_start, *, amplitude, h, ps, pw):
    """Device float64 ``n x 3``: per cell the sums (G, D, K) of DESIGN.md 4.16, the E-step of ``tl.cnv_states_fit``.
    ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W.  The launch is enqueued on the current
    stream; nothing is read back."""
    return _hmm_call(_lib.load().icv_posterior_stats, dm, chr_start, (amplitude, h, ps, pw), lambda torch: (
        torch.empty((dm.shape[0], 3), dtype=torch.float64, device="cuda"),))[0]


def _filter_call(entry, states, p_neutral, chr_start, thr, with_sign):
    """What :func:`states_filter` and :func:`copy_states_filter` share: ``entry(states, p_neutral, n, W, chr_start, C, thr,
    filtered, [sign,] nonneutral, removed, bad, stream)`` on the current stream.  Returns (filtered int8 n x W, [sign int8
    n x W,] nonneutral int32 n, removed int32 n, bad int32 flag), device tensors; nothing is read back."""
    torch = _torch()
    assert states.is_cuda and states.dtype == torch.int8 and states.dim() == 2 and states.is_contiguous()
    assert p_neutral.is_cuda and p_neutral.dtype == torch.float64 and p_neutral.is_contiguous()
    assert p_neutral.shape == states.shape and p_neutral.device == states.device
    n, w = int(states.shape[0]), int(states.shape[1])
    with torch.cuda.device(states.device):
        cs, n_chr = _chr_start_upload(torch, chr_start)
        planes = tuple(torch.empty((n, w), dtype=torch.int8, device="cuda") for _ in range(2 if with_sign else 1))
        count, removed = _empty(torch, n, torch.int32), _empty(torch, n, torch.int32)
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(entry(_ptr(states), _ptr(p_neutral), n, w, _ptr(cs), n_chr, float(thr), *(_ptr(t) for t in planes),
                         _ptr(count), _ptr(removed), _ptr(bad), _stream_ptr(torch)))
    return (*planes, count, removed, bad)


def states_filter(states, p_neutral, chr_start, max_p_normal):
    """(filtered int8 n x W, nonneutral int32 n, removed int32 n, bad int32 flag), device tensors: the calls of
    ``states`` (device int8) with every run whose mean ``p_neutral`` (device float64) is above ``max_p_normal`` reset to
    0 (the filter's rules 1-3).  Nothing is read back."""
    return _filter_call(_lib.load().icv_states_filter, states, p_neutral, chr_start, max_p_normal, False)


# ---- tl.cnv_copy_posteriors / tl.cnv_copy_states_filter: the K-state forward-backward chains and filter ----
def copy_posterior_chains(dm: DeviceMatrix, chr_start, *, levels, neutral, h, ps, pw, all_states=False):
    """(neutral, planes): device float64 ``n x W`` P(neutral) and, with ``all_states``, device float64 ``K x n x W`` with
    plane s = P(state s) (else None), by DESIGN.md 4.23 rules 2-6.  ``levels``: the K state means (host floats,
    ``levels[neutral] == 0``); ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W.  The launch
    is enqueued on the current stream; nothing is read back."""
    n, w = dm.shape
    return _hmm_call(_lib.load().icv_copy_posterior_chains, dm, chr_start, (*_levels_arg(levels, neutral), h, ps, pw),
                     lambda torch: (torch.empty((n, w), dtype=torch.float64, device="cuda"),
                                    torch.empty((len(levels), n, w), dtype=torch.float64, device="cuda")
                                    if all_states else None))


def copy_posterior_stats(dm: DeviceMatrix, chr_start, *, levels, neutral, h, ps, pw):
    """Device float64 ``n x (2K + 1)``: per cell the sums ``(N_0 .. N_{K-1}, M_0 .. M_{K-1}, S)`` of DESIGN.md 4.24, the
    E-step of ``tl.cnv_copy_states_fit``.  ``levels``: the K state means (host floats, ``levels[neutral] == 0``);
    ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W.  The launch is enqueued on the current
    stream; nothing is read back."""
    return _hmm_call(_lib.load().icv_copy_posterior_stats, dm, chr_start, (*_levels_arg(levels, neutral), h, ps, pw),
                     lambda torch: (torch.empty((dm.shape[0], 2 * len(levels) + 1), dtype=torch.float64, device="cuda"),))[0]


def copy_states_filter(states, p_neutral, chr_start, max_p_normal):
    """(filtered int8 n x W, sign int8 n x W, nonneutral int32 n, removed int32 n, bad int32 flag), device tensors: the
    levels of ``states`` (device int8, in [-7, 7]) with every run of one level whose mean ``p_neutral`` (device float64)
    is above ``max_p_normal`` reset to 0, and the same clipped to -1 / 0 / +1 (the filter's rules 1-3).
    Nothing is read back."""
    return _filter_call(_lib.load().icv_copy_states_filter, states, p_neutral, chr_start, max_p_normal, True)


# ---- tl.cnv_segments: runs of the int8 call matrix, group votes and consensus on the device (icv_segments_*, icv_state_*) --
def dense_input(x):
    """A dense array (the int8 calls, the float64 posteriors) as a contiguous CUDA tensor: a CUDA tensor is read where it
    lies, a host array is uploaded once.  (The caller checked shape and dtype.)"""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return x.cuda().contiguous()
    a = np.ascontiguousarray(x)
    if not a.flags.writeable:  # (torch does not wrap a read-only array)
        a = a.copy()
    return torch.from_numpy(a).cuda()


def segments_tables(states, chr_start):
    """The runs of every row of ``states`` (device int8 n x W; DESIGN.md 4.14 rules 1-2) as device tensors
    ``(counts int64 n, offsets int64 n + 1, row int64, start int32, end int32, state int8, bad int32 flag)``.
    ``chr_start``: host int32 array of C + 1 ascending window numbers from 0 to W.  One scalar (the number of segments)
    is read back between the count and the fill."""
    torch = _torch()
    lib = _lib.load()
    assert states.is_cuda and states.dtype == torch.int8 and states.dim() == 2 and states.is_contiguous()
    n, w = int(states.shape[0]), int(states.shape[1])
    with torch.cuda.device(states.device):
        st = _stream_ptr(torch)
        cs, n_chr = _chr_start_upload(torch, chr_start)
        counts = _empty(torch, n, torch.int64)
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.icv_segments_count(_ptr(states), n, w, _ptr(cs), n_chr, _ptr(counts), _ptr(bad), st))
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        _lib.check(lib.icv_row_offsets(_ptr(counts), n, _ptr(offsets), st))
        n_seg = int(offsets[-1].item())
        row, start, end, state = (_empty(torch, n_seg, t) for t in (torch.int64, torch.int32, torch.int32, torch.int8))
        _lib.check(lib.icv_segments_fill(_ptr(states), n, w, _ptr(cs), n_chr, _ptr(offsets), n_seg, _ptr(row), _ptr(start),
                                         _ptr(end), _ptr(state), st))
    return counts, offsets, row, start, end, state, bad


def state_votes(states, rows, group_ptr):
    """(loss, gain, bad): device int32 ``G x W`` counts of the listed rows of every group with -1 / +1 at each window
    (rule 4) and the device int32 bad-value flag.  ``rows``: host int64 row numbers sorted by group, ``group_ptr``: host
    int64 G + 1 positions.  Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    assert states.is_cuda and states.dtype == torch.int8 and states.dim() == 2 and states.is_contiguous()
    n, w = int(states.shape[0]), int(states.shape[1])
    assert int(group_ptr[0]) == 0 and int(group_ptr[-1]) == len(rows)
    with torch.cuda.device(states.device):
        d_rows, d_ptr, g = _group_lists_upload(torch, rows, group_ptr)
        loss = torch.empty((g, w), dtype=torch.int32, device="cuda")
        gain = torch.empty((g, w), dtype=torch.int32, device="cuda")
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.icv_state_votes(_ptr(states), n, w, _ptr(d_rows), int(d_rows.shape[0]), _ptr(d_ptr), g, _ptr(loss),
                                       _ptr(gain), _ptr(bad), _stream_ptr(torch)))
    return loss, gain, bad


def state_consensus(loss, gain, need):
    """Device int8 ``G x W`` consensus of rule 5; ``need``: host int32 per group."""
    torch = _torch()
    lib = _lib.load()
    g, w = int(loss.shape[0]), int(loss.shape[1])
    need = np.ascontiguousarray(need, dtype=np.int32)
    assert need.shape == (g,) and loss.dtype == torch.int32 and gain.dtype == torch.int32 and gain.shape == loss.shape
    with torch.cuda.device(loss.device):
        d_need = torch.from_numpy(need).cuda()
        consensus = torch.empty((g, w), dtype=torch.int8, device="cuda")
        _lib.check(lib.icv_state_consensus(_ptr(loss), _ptr(gain), _ptr(d_need), g, w, _ptr(consensus), _stream_ptr(torch)))
    return consensus


def segments_support(row, start, end, state, loss, gain):
    """(cells_min int32, cells_sum int64) of rule 6 for the segments of the consensus matrix, device tensors."""
    torch = _torch()
    lib = _lib.load()
    n_seg = int(row.shape[0])
    g, w = int(loss.shape[0]), int(loss.shape[1])
    with torch.cuda.device(loss.device):
        cells_min, cells_sum = _empty(torch, n_seg, torch.int32), _empty(torch, n_seg, torch.int64)
        _lib.check(lib.icv_segments_support(_ptr(row), _ptr(start), _ptr(end), _ptr(state), n_seg, _ptr(loss), _ptr(gain), g,
                                            w, _ptr(cells_min), _ptr(cells_sum), _stream_ptr(torch)))
    return cells_min, cells_sum


# ---- tl.cnv_copy_segments: the same for levels in [lo, hi], and the posterior sums of the runs (icv_level_*) --
def level_segments_tables(states, chr_start, lo, hi):
    """:func:`segments_tables` for levels: ``(counts, offsets, row, start, end, level int8, bad int32 flag)``, ``bad`` set
    where a value lies outside ``[lo, hi]``.  One scalar (the number of segments) is read back."""
    torch = _torch()
    lib = _lib.load()
    assert states.is_cuda and states.dtype == torch.int8 and states.dim() == 2 and states.is_contiguous()
    n, w = int(states.shape[0]), int(states.shape[1])
    with torch.cuda.device(states.device):
        st = _stream_ptr(torch)
        cs, n_chr = _chr_start_upload(torch, chr_start)
        counts = _empty(torch, n, torch.int64)
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.icv_level_segments_count(_ptr(states), n, w, _ptr(cs), n_chr, int(lo), int(hi), _ptr(counts),
                                                _ptr(bad), st))
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        _lib.check(lib.icv_row_offsets(_ptr(counts), n, _ptr(offsets), st))
        n_seg = int(offsets[-1].item())
        row, start, end, level = (_empty(torch, n_seg, t) for t in (torch.int64, torch.int32, torch.int32, torch.int8))
        _lib.check(lib.icv_level_segments_fill(_ptr(states), n, w, _ptr(cs), n_chr, _ptr(offsets), n_seg, _ptr(row),
                                               _ptr(start), _ptr(end), _ptr(level), st))
    return counts, offsets, row, start, end, level, bad


def level_votes(states, rows, group_ptr, lo, hi):
    """(counts, bad): device int32 ``G x (hi - lo + 1) x W`` counts of the listed rows of every group with level ``lo + p``
    at each window (rule 4) and the device int32 flag of a value outside ``[lo, hi]``.  ``rows`` / ``group_ptr`` as for
    :func:`state_votes`.  Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    assert states.is_cuda and states.dtype == torch.int8 and states.dim() == 2 and states.is_contiguous()
    n, w = int(states.shape[0]), int(states.shape[1])
    assert int(group_ptr[0]) == 0 and int(group_ptr[-1]) == len(rows)
    with torch.cuda.device(states.device):
        d_rows, d_ptr, g = _group_lists_upload(torch, rows, group_ptr)
        counts = torch.empty((g, int(hi) - int(lo) + 1, w), dtype=torch.int32, device="cuda")
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.icv_level_votes(_ptr(states), n, w, _ptr(d_rows), int(d_rows.shape[0]), _ptr(d_ptr), g, int(lo),
                                       int(hi), _ptr(counts), _ptr(bad), _stream_ptr(torch)))
    return counts, bad


def level_consensus(counts, need, lo, hi):
    """(loss int32 G x W, gain int32 G x W, consensus int8 G x W) of rule 5, device tensors; ``need``: host int32 per
    group."""
    torch = _torch()
    lib = _lib.load()
    g, w = int(counts.shape[0]), int(counts.shape[2])
    need = np.ascontiguousarray(need, dtype=np.int32)
    assert need.shape == (g,) and counts.dtype == torch.int32 and int(counts.shape[1]) == int(hi) - int(lo) + 1
    with torch.cuda.device(counts.device):
        d_need = torch.from_numpy(need).cuda()
        loss = torch.empty((g, w), dtype=torch.int32, device="cuda")
        gain = torch.empty((g, w), dtype=torch.int32, device="cuda")
        consensus = torch.empty((g, w), dtype=torch.int8, device="cuda")
        _lib.check(lib.icv_level_consensus(_ptr(counts), _ptr(d_need), g, w, int(lo), int(hi), _ptr(loss), _ptr(gain),
                                           _ptr(consensus), _stream_ptr(torch)))
    return loss, gain, consensus


def level_segments_support(row, start, end, level, counts, loss, gain, lo, hi):
    """(cells_min int32, cells_sum int64, level_min int32, level_sum int64) of rule 6 for the segments of the consensus
    matrix, device tensors."""
    torch = _torch()
    lib = _lib.load()
    n_seg = int(row.shape[0])
    g, w = int(loss.shape[0]), int(loss.shape[1])
    with torch.cuda.device(loss.device):
        cells_min, level_min = _empty(torch, n_seg, torch.int32), _empty(torch, n_seg, torch.int32)
        cells_sum, level_sum = _empty(torch, n_seg, torch.int64), _empty(torch, n_seg, torch.int64)
        _lib.check(lib.icv_level_segments_support(_ptr(row), _ptr(start), _ptr(end), _ptr(level), n_seg, _ptr(counts),
                                                  _ptr(loss), _ptr(gain), g, w, int(lo), int(hi), _ptr(cells_min),
                                                  _ptr(cells_sum), _ptr(level_min), _ptr(level_sum), _stream_ptr(torch)))
    return cells_min, cells_sum, level_min, level_sum


def segments_psum(p_neutral, row, start, end):
    """(psum int64 per segment, bad int32 flag), device tensors: the sum of ``rint(P 2^40)`` over every segment of the
    per-cell tables (rule 3); ``p_neutral``: device float64 ``n x W``.  Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    assert p_neutral.is_cuda and p_neutral.dtype == torch.float64 and p_neutral.dim() == 2 and p_neutral.is_contiguous()
    n, w = int(p_neutral.shape[0]), int(p_neutral.shape[1])
    n_seg = int(row.shape[0])
    with torch.cuda.device(p_neutral.device):
        psum = _empty(torch, n_seg, torch.int64)
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.icv_segments_psum(_ptr(p_neutral), n, w, _ptr(row), _ptr(start), _ptr(end), n_seg, _ptr(psum),
                                         _ptr(bad), _stream_ptr(torch)))
    return psum, bad


# ---- tl.cnv_pseudobulk: exact per-group mean profiles on the device (icv_group_profiles*) ------------------
def group_profiles(dm: DeviceMatrix, rows, group_ptr, shift):
    """(sum, stored, flags): device int64 / int32 ``G x W`` tables of rule 4 over the listed rows of every group and the
    device int32 flags (bit 0: a non-finite value, bit 1: a row number outside the matrix).  ``rows``: int64 row numbers
    sorted by group, ``group_ptr``: int64 G + 1 positions; host arrays are uploaded, CUDA tensors are used as they are.
    Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    with torch.cuda.device(dm.device):
        d_rows, d_ptr, g = _group_lists_upload(torch, rows, group_ptr)
        w = int(dm.shape[1])
        total = torch.empty((g, w), dtype=torch.int64, device="cuda")
        stored = torch.empty((g, w), dtype=torch.int32, device="cuda")
        flags = torch.empty(1, dtype=torch.int32, device="cuda")
        m = dm.c_struct()
        _lib.check(lib.icv_group_profiles(C.byref(m), _ptr(d_rows), int(d_rows.shape[0]), _ptr(d_ptr), g, int(shift),
                                          _ptr(total), _ptr(stored), _ptr(flags), _stream_ptr(torch)))
    return total, stored, flags, d_ptr


def group_profiles_finish(total, stored, d_ptr, shift):
    """(mean, fraction): device float64 ``G x W`` of rule 5 from the tables of :func:`group_profiles`; ``d_ptr`` is the
    device copy of ``group_ptr`` it returned.  Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    g, w = int(total.shape[0]), int(total.shape[1])
    with torch.cuda.device(total.device):
        mean = torch.empty((g, w), dtype=torch.float64, device="cuda")
        fraction = torch.empty((g, w), dtype=torch.float64, device="cuda")
        _lib.check(lib.icv_group_profiles_finish(_ptr(total), _ptr(stored), _ptr(d_ptr), g, w, int(shift), _ptr(mean),
                                                 _ptr(fraction), _stream_ptr(torch)))
    return mean, fraction


# ---- tl.cnv_pool_neighbors: exact means over every cell's graph neighbourhood (icv_neighbor_pool*) ----------
POOL_FLAG_NONFINITE, POOL_FLAG_COLUMN, POOL_FLAG_ORDER = 1, 2, 4


def neighbor_pool_graph(who, indptr, indices, data=None):
    """(indptr, indices): the structure of a device CSR graph as contiguous int64 / int32 CUDA tensors whose row pointers
    the kernels may trust (:func:`_graph_csr`); the ``indices`` of a graph without entries are one unused element, so that
    they have an address.  The values are not looked at beyond their number."""
    torch = _torch()
    if not (indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int64 and indices.dtype == torch.int32
            and indptr.dim() == 1 and indices.dim() == 1):
        raise ValueError(f"{who}: a device graph is (indptr int64, indices int32, data) of 1-D CUDA tensors")
    if data is not None and data.numel() != indices.numel():
        raise ValueError(f"{who}: the graph has {indices.numel()} columns and {data.numel()} values")
    indptr, indices, _, _, nnz = _graph_csr(who, indptr, indices, indices, (torch.int32,))
    if nnz == 0:  # (a tensor of no elements has no address: one element that nothing reads)
        indices = torch.zeros(1, dtype=torch.int32, device=indptr.device)
    return indptr, indices


def neighbor_pool_sizes(indptr, indices):
    """(n_cells, flags): the device int32 sizes L_i of rule 2 and the device int32 flag word (POOL_FLAG_COLUMN: a column
    outside [0, n); POOL_FLAG_ORDER: a row that does not ascend strictly) of the graph of :func:`neighbor_pool_graph`.
    Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    n = int(indptr.numel()) - 1
    with torch.cuda.device(indptr.device):
        n_cells = torch.empty(n, dtype=torch.int32, device="cuda")
        flags = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.icv_neighbor_pool_sizes(_ptr(indptr), _ptr(indices), n, _ptr(n_cells), _ptr(flags),
                                               _stream_ptr(torch)))
    return n_cells, flags


def neighbor_pool(dm: DeviceMatrix, indptr, indices, shift, n_cells, flags, out=None):
    """The device float64 ``n x W`` matrix of rules 1, 4 and 5 for ``dm`` and the graph and sizes of
    :func:`neighbor_pool_sizes`; POOL_FLAG_NONFINITE is added to ``flags`` where a value is not finite.  ``out``: a
    contiguous result to write into.  Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    n, w = int(dm.shape[0]), int(dm.shape[1])
    with torch.cuda.device(dm.device):
        if out is None:
            out = torch.empty((n, w), dtype=torch.float64, device="cuda")
        assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n, w) and out.is_contiguous()
        m = dm.c_struct()
        _lib.check(lib.icv_neighbor_pool(C.byref(m), _ptr(indptr), _ptr(indices), int(indptr.numel()) - 1, int(shift),
                                         _ptr(n_cells), _ptr(out), w, _ptr(flags), _stream_ptr(torch)))
    return out


# ---- tl.cnv_correlation / tl.cnv_signal: rows against centred profiles on the device (icv_profile_corr*) ------
def profile_corr(dm: DeviceMatrix, centred=None, s2=None):
    """(A, B, signal, r, flags): device float64 vectors of rule 2's row sums and of ``B / W``, the device float64 ``n x G``
    correlations of rule 3 and the device int32 flags (bit 0: a non-finite stored value).  ``centred``: host float64
    ``G x W`` centred profiles, ``s2``: host float64 ``G`` sums of squares; both None gives G = 0 and an ``n x 0`` r.
    Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    n, w = int(dm.shape[0]), int(dm.shape[1])
    with torch.cuda.device(dm.device):
        if centred is None:
            g, ct, d_s2 = 0, None, None
        else:
            centred = np.asarray(centred, dtype=np.float64)
            g = int(centred.shape[0])
            assert centred.shape == (g, w) and np.asarray(s2).shape == (g,)
            ct = torch.from_numpy(np.ascontiguousarray(centred.T)).cuda()  # (W x G: a window's values are contiguous)
            d_s2 = torch.from_numpy(np.ascontiguousarray(s2, dtype=np.float64)).cuda()
        a, b, signal = (_empty(torch, n, torch.float64) for _ in range(3))
        r = _empty(torch, n * g, torch.float64).reshape(n, g)
        flags = torch.empty(1, dtype=torch.int32, device="cuda")
        m = dm.c_struct()
        _lib.check(lib.icv_profile_corr(C.byref(m), _ptr(ct) if g else None, _ptr(d_s2) if g else None, g, _ptr(a), _ptr(b),
                                        _ptr(signal), _ptr(r) if g else None, _ptr(flags), _stream_ptr(torch)))
    return a, b, signal, r, flags


def profile_corr_best(r):
    """(best_r float64 n, best_g int32 n), device tensors: rule 4 for the device ``n x G`` table of :func:`profile_corr`.
    Nothing is read back."""
    torch = _torch()
    lib = _lib.load()
    assert r.is_cuda and r.dtype == torch.float64 and r.dim() == 2 and r.is_contiguous()
    n, g = int(r.shape[0]), int(r.shape[1])
    with torch.cuda.device(r.device):
        best_r, best_g = _empty(torch, n, torch.float64), _empty(torch, n, torch.int32)
        _lib.check(lib.icv_profile_corr_best(_ptr(r) if g else None, n, g, _ptr(best_r), _ptr(best_g), _stream_ptr(torch)))
    return best_r, best_g


# ---- tl.cnv_silhouette: int64 sums of rounded distances and the widths on the device (icv_silhouette_*) -------
SILHOUETTE_TILE_I = _lib.ICV_SILHOUETTE_TILE_I  # positions i of a workgroup; the row slabs of S are multiples of it
SILHOUETTE_TILE_J = _lib.ICV_SILHOUETTE_TILE_J  # positions of a j-tile; a tile never straddles a group
SILHOUETTE_TILE_C = _lib.ICV_SILHOUETTE_TILE_C  # components per LDS stage
SILHOUETTE_MAX_COMPONENTS = _lib.ICV_SILHOUETTE_MAX_COMPONENTS
SILHOUETTE_MAX_SHIFT = _lib.ICV_SILHOUETTE_MAX_SHIFT
SILHOUETTE_S_BUDGET = 1 << 30  # bytes of the int64 table S above which it is formed in row slabs
SILHOUETTE_TARGET_BLOCKS = 2048  # workgroups a launch aims for (8 per CU of 256): the j-tiles are cut into chunks for it
SILHOUETTE_STAGES = ("sums", "finish")


def silhouette_tiles(group_ptr, n_chunks):
    """(tiles, chunk_ptr) for ``group_ptr`` (host int64, G + 1): the int64 ``3 x T`` table of the j-tiles -- first
    position, number of positions, group; at most ``SILHOUETTE_TILE_J`` positions each, none straddling a group, in
    position order -- and the int32 ``n + 1`` tile numbers that cut them into ``n = min(max(n_chunks, 1), T, 65535)``
    consecutive chunks of as equal a number of tiles as possible."""
    group_ptr = np.asarray(group_ptr, dtype=np.int64)
    sizes = np.diff(group_ptr)
    per_group = -(-sizes // SILHOUETTE_TILE_J)
    group = np.repeat(np.arange(sizes.shape[0], dtype=np.int64), per_group)
    n_tiles = int(group.shape[0])
    first_tile = np.concatenate([[0], np.cumsum(per_group)])[:-1]
    k = np.arange(n_tiles, dtype=np.int64) - first_tile[group]  # the tile's number inside its group
    start = group_ptr[group] + k * SILHOUETTE_TILE_J
    count = np.minimum(group_ptr[group + 1] - start, SILHOUETTE_TILE_J)
    n = min(max(int(n_chunks), 1), max(n_tiles, 1), 65535)
    chunk_ptr = (np.arange(n + 1, dtype=np.int64) * n_tiles // n).astype(np.int32)
    return np.ascontiguousarray(np.stack([start, count, group])), chunk_ptr


def silhouette(dm: DeviceMatrix, rows, group_ptr, shift, dist_exp, *, s_budget=None, n_chunks=None, stage_ms=None):
    """(s, a, b, nearest, flags): device float64 / int32 vectors of DESIGN.md 4.26 rules 3-5 for the labelled cells BY
    POSITION (``rows``, host int64: the rows of ``dm`` sorted by group, ascending inside a group; ``group_ptr``, host
    int64 G + 1: the first position of every group) and the device int32 flag word (bit 0: a non-finite value).
    ``shift``: rule 2's e; ``dist_exp``: every distance is below 2^dist_exp.  ``s_budget``: bytes of the int64 table S
    (default ``SILHOUETTE_S_BUDGET``): above it S is formed and used in slabs of rows, a multiple of
    ``SILHOUETTE_TILE_I`` each (never fewer: a budget below one tile's rows gives slabs of one tile).  ``n_chunks``: the
    chunks the j-tiles are cut into (default: what gives ``SILHOUETTE_TARGET_BLOCKS`` workgroups per launch).  Neither
    changes a bit of the result.  ``stage_ms``: a dict that receives the device-event milliseconds of
    ``SILHOUETTE_STAGES`` (one synchronisation at the end).  Nothing else is read back."""
    torch = _torch()
    lib = _lib.load()
    assert dm.format == _lib.ICV_DENSE
    n, c = int(dm.shape[0]), int(dm.shape[1])
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    group_ptr = np.ascontiguousarray(group_ptr, dtype=np.int64)
    m, g = int(rows.shape[0]), int(group_ptr.shape[0]) - 1
    assert g >= 1 and int(group_ptr[0]) == 0 and int(group_ptr[-1]) == m and (np.diff(group_ptr) >= 0).all()
    assert m == 0 or (0 <= int(rows.min()) and int(rows.max()) < n)
    budget = SILHOUETTE_S_BUDGET if s_budget is None else int(s_budget)
    slab = max(budget // (8 * g) // SILHOUETTE_TILE_I, 1) * SILHOUETTE_TILE_I
    slab = min(slab, -(-max(m, 1) // SILHOUETTE_TILE_I) * SILHOUETTE_TILE_I)
    if n_chunks is None:
        n_chunks = -(-SILHOUETTE_TARGET_BLOCKS // (min(slab, max(m, 1)) // SILHOUETTE_TILE_I + 1))
    tiles, chunk_ptr = silhouette_tiles(group_ptr, n_chunks)
    marks = []

    def mark(name):
        if stage_ms is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name, ev))

    with torch.cuda.device(dm.device):
        st = _stream_ptr(torch)
        d_rows = torch.from_numpy(rows).cuda() if m else torch.zeros(1, dtype=torch.int64, device="cuda")
        d_ptr = torch.from_numpy(group_ptr).cuda()
        d_tiles = torch.from_numpy(tiles).cuda() if tiles.shape[1] else torch.zeros(3, dtype=torch.int64, device="cuda")
        d_chunks = torch.from_numpy(chunk_ptr).cuda()
        sums = torch.empty(max(min(slab, m), 1) * g, dtype=torch.int64, device="cuda")
        s, a, b = (_empty(torch, m, torch.float64) for _ in range(3))
        nearest = _empty(torch, m, torch.int32)
        flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        x = dm.dense
        dtype = _lib.ICV_F32 if x.dtype == torch.float32 else _lib.ICV_F64
        for i0 in range(0, m, slab):
            i1 = min(i0 + slab, m)
            mark(None)
            _lib.check(lib.icv_silhouette_sums(_ptr(x), dtype, n, c, int(x.stride(0)) if n > 1 else c, _ptr(d_rows), m, i0,
                                               i1, _ptr(d_tiles), int(tiles.shape[1]), _ptr(d_chunks),
                                               int(chunk_ptr.shape[0]) - 1, g, int(shift), int(dist_exp), _ptr(sums),
                                               _ptr(flags), st))
            mark("sums")
            _lib.check(lib.icv_silhouette_finish(_ptr(sums), i0, i1, _ptr(d_ptr), g, int(shift), _ptr(s), _ptr(a), _ptr(b),
                                                 _ptr(nearest), st))
            mark("finish")
        if stage_ms is not None:
            torch.cuda.current_stream().synchronize()
            for (_, e0), (name, e1) in zip(marks, marks[1:]):
                if name is not None:
                    stage_ms[name] = stage_ms.get(name, 0.0) + float(e0.elapsed_time(e1))
    return s, a, b, nearest, flags


# ---- tl.cnv_kmeans: seeding, assignment and integer update on the device (icv_kmeans_*) -------------------
KMEANS_MAX_COMPONENTS = _lib.ICV_KMEANS_MAX_COMPONENTS
KMEANS_MAX_CLUSTERS = _lib.ICV_KMEANS_MAX_CLUSTERS
KMEANS_MAX_SHIFT = _lib.ICV_KMEANS_MAX_SHIFT
KMEANS_FLAG_NONFINITE, KMEANS_FLAG_NO_MASS = 1, 2
KMEANS_STAGES = ("seed", "lloyd")


def kmeans(dm: DeviceMatrix, k, shift_e, shift_f, max_iter, *, draws=None, init=None, stage_ms=None):
    """The runs of DESIGN.md 4.27 rules 4-8 on ``dm`` (dense n x C).  ``draws``: per run the k hash values ``z_0 .. z_{k-1}``
    of rule 3 (Python ints below 2^64); or ``init``, a host float64 k x C table of starting centres, for one run without
    seeding.  Returns a dict: ``labels`` (device int32 n), ``sqdist`` (device float64 n: D(i, label_i)) and ``centres``
    (device float64 k x C) of the run of lowest integer inertia (ties: the first), in the raw cluster order;
    ``best``, ``n_iter``, ``converged`` and ``inertia_q`` (per run) of the host; ``history`` (per run, the
    (inertia, n_changed) of every iteration) and ``picks`` (per run the k seeded rows, None with ``init``).  One copy of
    three words (inertia, n_changed, flag word) comes back per iteration, as the Baum-Welch fits read their sums; the
    picks come back once at the end.  ``ValueError`` for a non-finite value that a kernel read and for seeding weights that
    add up to 0 (fewer distinct points than clusters).  ``stage_ms``: a dict that receives host-clock milliseconds of
    ``KMEANS_STAGES`` (``seed`` only enqueues; ``lloyd`` ends in the read-backs)."""
    torch = _torch()
    lib = _lib.load()
    assert dm.format == _lib.ICV_DENSE and (draws is None) != (init is None)
    n, c = int(dm.shape[0]), int(dm.shape[1])
    k = int(k)
    x = dm.dense
    dtype = _lib.ICV_F32 if x.dtype == torch.float32 else _lib.ICV_F64
    ld = int(x.stride(0)) if n > 1 else c
    n_runs = 1 if draws is None else len(draws)
    seed_blocks = -(-n // _lib.ICV_KMEANS_SEED_ROWS)
    clock = {name: 0.0 for name in KMEANS_STAGES}

    with torch.cuda.device(dm.device):
        st = _stream_ptr(torch)
        head = (_ptr(x), dtype, n, c, ld)
        # words 0, 1: the inertia and n_changed of the last assignment; the low half of word 2: the flag word
        state = torch.zeros(3, dtype=torch.int64, device="cuda")
        flags = state[2:].view(torch.int32)
        sums = torch.empty(k * (c + 1), dtype=torch.int64, device="cuda")
        picks = torch.full((n_runs, k), -1, dtype=torch.int64, device="cuda")
        if draws is not None:
            mind = torch.empty(n, dtype=torch.float64, device="cuda")
            w = torch.empty(n, dtype=torch.int64, device="cuda")
            partials = torch.empty(seed_blocks, dtype=torch.int64, device="cuda")
        best, kept = -1, None
        inertia_q, n_iters, converged, history = [], [], [], []
        for r in range(n_runs):
            t0 = _time.perf_counter()
            labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            sqdist = torch.empty(n, dtype=torch.float64, device="cuda")
            if draws is None:
                centres = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64)).cuda()
            else:
                centres = torch.zeros((k, c), dtype=torch.float64, device="cuda")
                for t in range(k):
                    if t:
                        _lib.check(lib.icv_kmeans_seed_dist(*head, C.c_void_p(centres.data_ptr() + 8 * c * (t - 1)), int(t == 1),
                                                            int(shift_f), _ptr(mind), _ptr(w), _ptr(partials), _ptr(flags), st))
                    _lib.check(lib.icv_kmeans_seed_pick(*head, _ptr(w) if t else None, _ptr(partials) if t else None, t, k,
                                                        int(draws[r][t]), _ptr(centres), _ptr(picks[r]), _ptr(flags), st))
            t1 = _time.perf_counter()
            clock["seed"] += t1 - t0
            trace = []
            it = 0
            while True:
                it += 1
                _lib.check(lib.icv_kmeans_assign(*head, _ptr(centres), k, int(shift_f), _ptr(labels), _ptr(sqdist),
                                                 _ptr(state), _ptr(flags), st))
                inertia, changed, flag = (int(v) for v in state.cpu().tolist())
                if flag & KMEANS_FLAG_NO_MASS:
                    raise ValueError(f"the rows hold fewer than {k} distinct points")
                if flag & KMEANS_FLAG_NONFINITE:
                    raise ValueError("non-finite values")
                trace.append((inertia, changed))
                if changed == 0 or it == max_iter:
                    break
                _lib.check(lib.icv_kmeans_update(*head, _ptr(labels), k, int(shift_e), _ptr(sums), st))
                _lib.check(lib.icv_kmeans_centres(_ptr(sums), k, c, int(shift_e), _ptr(centres), st))
            clock["lloyd"] += _time.perf_counter() - t1
            history.append(trace)
            inertia_q.append(trace[-1][0])
            n_iters.append(it)
            converged.append(trace[-1][1] == 0)
            if best < 0 or inertia_q[r] < inertia_q[best]:
                best, kept = r, (labels, sqdist, centres)
        host_picks = picks.cpu().numpy() if draws is not None else None
    if stage_ms is not None:
        for name in KMEANS_STAGES:
            stage_ms[name] = stage_ms.get(name, 0.0) + clock[name] * 1e3
    return {"labels": kept[0], "sqdist": kept[1], "centres": kept[2], "best": best, "n_iter": n_iters,
            "converged": converged, "inertia_q": inertia_q, "history": history,
            "picks": None if host_picks is None else [row.tolist() for row in host_picks]}


# ---- tl.cnv_rank_groups: exact doubled mid-rank sums on the device (icv_rank_*) ---------------------------
RANK_STAGES = ("count", "scatter", "sort", "rank_sums", "finish")


def rank_window_tiles(counts, max_entries):
    """[(w0, w1), ...]: the windows cut into consecutive tiles whose ``counts`` (host int64 per window) sum to at most
    ``max_entries``; a tile has at least one window, whatever its count."""
    ends = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    tiles, w0, n_windows = [], 0, int(counts.shape[0])
    while w0 < n_windows:
        w1 = int(np.searchsorted(ends, ends[w0] + int(max_entries), side="right")) - 1
        w1 = min(n_windows, max(w1, w0 + 1))
        tiles.append((w0, w1))
        w0 = w1
    return tiles


def rank_tables(dm: DeviceMatrix, code, n_cells, *, max_entries=1 << 28, stage_ms=None, info=None):
    """(R2, T, flags): device int64 ``G x W`` and ``W`` tables of DESIGN.md 4.20 rule 2 and the flag word as an int (bit
    0: a value of the population is not finite; R2 and T are None then and nothing but the count has run).  ``code``:
    host int32 per row, -1 outside the population, 0 .. G - 1 for the G tested groups, G for the cells that are ranked
    but belong to no tested group; ``n_cells``: host int64 sizes of the G groups.  The windows are ranked in consecutive
    tiles of at most ``max_entries`` ranked values (never below the population, so that a window always fits), which
    bounds the workspace at 24 bytes per entry of the largest tile; ``MemoryError`` when that does not fit the free
    HBM.  The window counts and the flag word are read back in one copy.  ``stage_ms``: a dict that receives the
    device-event milliseconds of ``RANK_STAGES`` (one more synchronisation at the end); ``info``: a dict that receives
    ``n_entries`` and ``n_tiles``."""
    torch = _torch()
    lib = _lib.load()
    n, w = int(dm.shape[0]), int(dm.shape[1])
    code = np.ascontiguousarray(code, dtype=np.int32)
    n_cells = np.ascontiguousarray(n_cells, dtype=np.int64)
    g = int(n_cells.shape[0])
    n_pop = int(np.count_nonzero(code >= 0))
    assert code.shape == (n,) and g >= 1 and int(code.max(initial=-1)) <= g
    if n_pop >= _lib.ICV_RANK_MAX_CELLS:
        raise ValueError(f"rank_tables: {n_pop} cells are ranked against each other; at most {_lib.ICV_RANK_MAX_CELLS - 1} "
                         f"are supported (N^3 in an int64)")
    marks = []

    def mark(name):
        if stage_ms is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name, ev))

    with torch.cuda.device(dm.device):
        st = _stream_ptr(torch)
        m = dm.c_struct()
        d_code = torch.from_numpy(code).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
        head = torch.empty(1 + w, dtype=torch.int32, device="cuda")  # the flag word, then the window counts
        flags, stored = head[:1], head[1:]
        mark(None)
        _lib.check(lib.icv_rank_count(C.byref(m), _ptr(d_code), _ptr(stored), _ptr(flags), st))
        mark("count")
        host = head.cpu().numpy()
        bits, counts = int(host[0]), host[1:].astype(np.int64)
        if bits & 1:
            return None, None, bits
        cap = min(max(int(max_entries), n_pop, 1), 2 ** 31 - 1)
        tiles = rank_window_tiles(counts, cap)
        ends = np.concatenate([[0], np.cumsum(counts)])
        largest = max(int(ends[w1] - ends[w0]) for w0, w1 in tiles)
        need = 24 * largest + (g + 1) * w * 12 + w * 12
        if need > free_hbm_bytes():
            raise MemoryError(f"rank_tables: the workspace of {largest} ranked values per window tile and the tables of "
                              f"{g + 1} x {w} sums take {need} bytes, more than the {free_hbm_bytes()} bytes of free HBM; "
                              f"lower max_entries (now {cap})")
        r2 = torch.zeros((g + 1, w), dtype=torch.int64, device="cuda")
        cnt = torch.zeros((g + 1, w), dtype=torch.int32, device="cuda")
        tie = torch.zeros(w, dtype=torch.int64, device="cuda")
        neg = torch.zeros(w, dtype=torch.int32, device="cuda")
        keys = torch.empty((2, max(largest, 1)), dtype=torch.int64, device="cuda")  # (uint64 keys, as bits)
        payload = torch.empty((2, max(largest, 1)), dtype=torch.int32, device="cuda")
        d_cells = torch.from_numpy(n_cells).cuda()
        for w0, w1 in tiles:
            n_entries = int(ends[w1] - ends[w0])
            if n_entries == 0:
                continue
            seg = torch.from_numpy((ends[w0:w1 + 1] - ends[w0]).astype(np.int32)).cuda()
            cursor = torch.empty(w1 - w0, dtype=torch.int32, device="cuda")
            mark(None)
            _lib.check(lib.icv_rank_scatter(C.byref(m), _ptr(d_code), w0, w1 - w0, _ptr(seg), _ptr(cursor), _ptr(keys[0]),
                                            _ptr(payload[0]), st))
            mark("scatter")
            _lib.check(lib.icv_rank_sort(_ptr(keys[0]), _ptr(payload[0]), n_entries, _ptr(seg), w1 - w0, _ptr(keys[1]),
                                         _ptr(payload[1]), st))
            mark("sort")
            _lib.check(lib.icv_rank_sums(_ptr(keys[1]), _ptr(payload[1]), _ptr(seg), w0, w1 - w0, int(counts[w0:w1].max()),
                                         w, n_pop, g + 1, _ptr(r2), _ptr(cnt), _ptr(tie), _ptr(neg), st))
            mark("rank_sums")
        mark(None)
        _lib.check(lib.icv_rank_finish(_ptr(stored), _ptr(neg), _ptr(cnt), _ptr(d_cells), g, w, n_pop, _ptr(r2), _ptr(tie), st))
        mark("finish")
        if stage_ms is not None:
            torch.cuda.current_stream().synchronize()
            for (_, a), (name, b) in zip(marks, marks[1:]):
                if name is not None:
                    stage_ms[name] = stage_ms.get(name, 0.0) + float(a.elapsed_time(b))
    if info is not None:
        info.update(n_entries=int(ends[-1]), n_tiles=len(tiles))
    return r2[:g], tie, bits

"""The two pure rules of the ``tl.infercnv`` driver, on the CPU: the compute dtype and kernel flags of a host matrix as a
literal table, and the slab / piece sizing of the host path and of the resident path."""
import numpy as np
import pytest

# ----------------------------------------------------------------------------------------------------------------------
# the compute dtype and the kernel flags: what numpy's promotion gives the reference, written out
# ----------------------------------------------------------------------------------------------------------------------
F32, F64 = np.float32, np.float64
# matrix dtype -> for reference (None | float32 | float64) x (1 row | 2 rows): (compute dtype, flag name | None)
DTYPE_TABLE = {
    np.bool_:   {(None, 1): (F64, None), (F32, 1): (F64, None), (F64, 1): (F64, None),
                 (F32, 2): (F64, "TRUNC"), (F64, 2): (F64, "TRUNC")},
    np.uint8:   {(None, 1): (F64, None), (F32, 1): (F64, None), (F64, 1): (F64, None),
                 (F32, 2): (F64, "TRUNC"), (F64, 2): (F64, "TRUNC")},
    np.int32:   {(None, 1): (F64, None), (F32, 1): (F64, None), (F64, 1): (F64, None),
                 (F32, 2): (F64, "TRUNC"), (F64, 2): (F64, "TRUNC")},
    np.int64:   {(None, 1): (F64, None), (F32, 1): (F64, None), (F64, 1): (F64, None),
                 (F32, 2): (F64, "TRUNC"), (F64, 2): (F64, "TRUNC")},
    # (the means of a float16 matrix are formed in float64: without a given reference it computes in float64)
    np.float16: {(None, 1): (F64, None), (F32, 1): (F32, None), (F64, 1): (F64, None),
                 (F32, 2): (F32, None), (F64, 2): (F64, "ROUND")},
    np.float32: {(None, 1): (F32, None), (F32, 1): (F32, None), (F64, 1): (F64, None),
                 (F32, 2): (F32, None), (F64, 2): (F64, "ROUND")},
    np.float64: {(None, 1): (F64, None), (F32, 1): (F64, None), (F64, 1): (F64, None),
                 (F32, 2): (F64, None), (F64, 2): (F64, None)},
}


def test_compute_dtype_and_flags_table():
    from infercnvpy_amd import _lib
    from infercnvpy_amd.tl import _infercnv as T

    flag = {None: 0, "TRUNC": _lib.ICV_FLAG_TRUNC_TO_INT, "ROUND": _lib.ICV_FLAG_ROUND_F32}
    assert flag["TRUNC"] and flag["ROUND"] and flag["TRUNC"] != flag["ROUND"]
    for x_dtype, row in DTYPE_TABLE.items():
        assert len(row) == 5
        for (ref_dtype, n_rows), (compute, name) in row.items():
            got = T._compute_dtype(np.dtype(x_dtype), None if ref_dtype is None else np.dtype(ref_dtype), n_rows)
            assert got == (compute, flag[name]), (x_dtype, ref_dtype, n_rows, got)
            # means formed from the matrix: as many rows as categories, the same rule
            if ref_dtype is None:
                exp2 = (compute, flag["TRUNC"] if np.dtype(x_dtype).kind in "iub" else
                        flag["ROUND"] if x_dtype is np.float16 else 0)
                assert T._compute_dtype(np.dtype(x_dtype), None, 3) == exp2
    for bad in (np.complex64, np.complex128, np.dtype("O"), np.dtype("U3"), np.dtype("M8[s]")):
        with pytest.raises(ValueError) as err:
            T._compute_dtype(np.dtype(bad), None, 1)
        assert str(err.value) == f"unsupported matrix dtype {np.dtype(bad)}"


# ----------------------------------------------------------------------------------------------------------------------
# slab and piece sizing
# ----------------------------------------------------------------------------------------------------------------------
def test_host_row_bytes():
    from infercnvpy_amd.tl import _infercnv as T

    # dense float32, 1000 genes, 91 windows: 4000 (row) + 364 (x_res) + 64 + 728 (float64 window scratch)
    assert T._host_row_bytes(1000, 91, 4, False) == 5156
    # + float64 gene matrix, float64 windows, covered-gene means
    assert T._host_row_bytes(1000, 91, 4, True) == 5156 + 8 * 2091 + 364
    # CSR float64, 12.5 stored entries per row: 12 bytes each + the row offset
    assert T._host_row_bytes(1000, 91, 8, False, stored_per_row=12.5) == 12.5 * 12 + 8 + 364 + 64 + 728
    assert T._host_row_bytes(1000, 91, 8, False, stored_per_row=0.0) == 12 + 8 + 364 + 64 + 728  # (at least one entry)


def _check_sizing(T, n_rows, chunksize, **kw):
    piece_rows, slabs = T._host_sizing(n_rows, chunksize=chunksize, **kw)
    assert piece_rows >= chunksize and piece_rows % chunksize == 0
    if n_rows == 0:
        assert slabs == []
        return piece_rows, slabs
    assert slabs[0][0] == 0 and slabs[-1][1] == n_rows
    for (a0, a1), (b0, b1) in zip(slabs[:-1], slabs[1:]):
        assert a1 == b0 and a0 < a1
    slab_rows = slabs[0][1] - slabs[0][0]
    assert all(b - a == slab_rows for a, b in slabs[:-1]) and 0 < slabs[-1][1] - slabs[-1][0] <= slab_rows
    assert len(slabs) == 1 or (slab_rows % chunksize == 0 and slab_rows >= chunksize)
    return piece_rows, slabs


def test_host_sizing_properties():
    from infercnvpy_amd.tl import _infercnv as T

    rng = np.random.RandomState(5)
    for _ in range(300):
        chunksize = int(rng.choice([1, 7, 100, 5000]))
        n_rows = int(rng.choice([0, 1, chunksize - 1, chunksize, 3 * chunksize + 1, int(rng.randint(1, 2_000_000))]))
        n_rows = max(n_rows, 0)
        _check_sizing(T, n_rows, chunksize, per_row=float(rng.choice([1.0, 77.5, 5156, 81_000])),
                      free_bytes=int(rng.choice([0, 1 << 20, 1 << 30, 200 << 30])), share=int(rng.randint(1, 4)),
                      n_windows=int(rng.choice([1, 91, 1993])), piece_bytes=float(rng.choice([1.0, 5e6, 2e9])))


def test_host_sizing_literal_cases():
    """The first case can be checked by hand (2e9 // 5156 = 387 897 rows, rounded down to whole 5000-cell chunks; the
    slab: 0.45 * 200 GiB less 3 pieces of packed results, over 5156 bytes per row, holds all rows).  The expected numbers
    of the other three were obtained by evaluating the expressions of the driver before it had these functions."""
    from infercnvpy_amd.tl import _infercnv as T

    kw = dict(per_row=5156, free_bytes=200 << 30, share=1, chunksize=5000, n_windows=91, piece_bytes=2e9)
    assert _check_sizing(T, 200_000, **kw) == (385_000, [(0, 200_000)])
    # bench.py's host call: dense float32, 20 000 genes, 1993 windows, two shards on one GPU with 250 GiB free
    kw = dict(per_row=T._host_row_bytes(20_000, 1993, 4, False), free_bytes=250 << 30, share=2, chunksize=5000,
              n_windows=1993, piece_bytes=2e9)
    assert kw["per_row"] == 103_980
    assert _check_sizing(T, 100_000, **kw) == (15_000, [(0, 100_000)])
    # little memory: several slabs, the last one short
    kw = dict(per_row=103_980, free_bytes=8 << 30, share=1, chunksize=5000, n_windows=1993, piece_bytes=2e9)
    assert _check_sizing(T, 100_000, **kw) == (15_000, [(0, 25_000), (25_000, 50_000), (50_000, 75_000), (75_000, 100_000)])
    # no room at all, a piece smaller than a chunk: one chunk per piece and per slab
    kw = dict(per_row=81_000.5, free_bytes=0, share=3, chunksize=100, n_windows=500, piece_bytes=5e6)
    assert _check_sizing(T, 250, **kw) == (100, [(0, 100), (100, 200), (200, 250)])


def test_resident_piece_rows():
    """Whole chunks whose result buffers fit into 40 % of the free memory; with gene values the float64 gene matrix of
    all rows is set aside first (never more than 7/8 of what is free).  Numbers from the driver's earlier expressions."""
    from infercnvpy_amd.tl import _infercnv as T

    # 16 * 1993 + 64 = 31 952 bytes per row; 0.4 * 250 GiB // 31 952 = 3 360 483 rows -> 3 360 000
    assert T._resident_piece_rows(100_000, 20_000, 1993, 250 << 30, 5000, False) == 3_360_000
    # gene values: 31 952 + 8 * 21 993 = 207 896 per row; (250 GiB - 16 GB) * 0.4 // 207 896 = 485 695 rows -> 485 000
    assert T._resident_piece_rows(100_000, 20_000, 1993, 250 << 30, 5000, True) == 485_000
    # the gene matrix alone exceeds what is free: an eighth of it is planned with
    assert T._resident_piece_rows(1_000_000, 20_000, 1993, 100 << 30, 5000, True) == 25_000
    assert T._resident_piece_rows(1000, 20_000, 1993, 0, 300, False) == 300  # never less than one chunk
    for cs in (1, 7, 5000):
        for free_b in (0, 1 << 30, 250 << 30):
            p = T._resident_piece_rows(123_457, 2000, 191, free_b, cs, True)
            assert p >= cs and p % cs == 0

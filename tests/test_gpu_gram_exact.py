"""Bit-exact tests of the fp32 MFMA Gram as squared distances (``icv_pairwise_sqeuclidean`` and the sharded tile
entry ``icv_pairwise_sqeuclidean_tiles``) on integer inputs where float32 makes no rounding error
(tests/_exact_inputs.py): every entry must equal the exact int64 distance.

test_gpu_parity.py holds the same kernels to 1e-5 relative against float64 numpy, and the sharded tiles only
through the Ward linkage they feed."""
import numpy as np
import pytest

import _exact_inputs as E

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (3, 5), (127, 16), (128, 17), (129, 143), (1023, 160), (1024, 161), (1025, 288),
          (2049, 1802)]


def _gpu(X):
    import torch

    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()


def _exact32(Zc, rows=None):
    D = E.exact_sqdist(Zc, rows)
    assert D.max(initial=0) < 2 ** 24  # so float32 holds it exactly
    return D.astype(np.float32)


@pytest.mark.parametrize("n,d", SHAPES)
def test_pairwise_full_exact(n, d):
    from infercnvpy_amd import _engine

    X, Zc = E.dist_case(n, d, seed=n * 7 + d, dup=n // 50)
    got = _engine.pairwise_sqeuclidean(_gpu(X)).cpu().numpy()
    exp = _exact32(Zc)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(got, got.T)
    assert (np.diag(got) == 0).all()
    if n >= 50:  # duplicate rows: exact zeros off the diagonal
        assert (got[~np.eye(n, dtype=bool)] == 0).sum() >= 2 * (n // 50)


@pytest.mark.parametrize("n,d", [(2049, 161), (3000, 17)])
def test_pairwise_row_blocks_exact(n, d):
    """Row blocks starting on and off the 1024-row super-tile boundary."""
    from infercnvpy_amd import _engine

    X, Zc = E.dist_case(n, d, seed=n + d, dup=5)
    xd = _gpu(X)
    for r0, r1 in ((0, 1), (100, 389), (1023, 1025), (1024, 2048), (n - 1, n), (0, n)):
        got = _engine.pairwise_sqeuclidean(xd, rows=(r0, r1)).cpu().numpy()
        np.testing.assert_array_equal(got, _exact32(Zc, np.arange(r0, r1)), err_msg=f"rows {r0}:{r1}")


def test_pairwise_strided_out_and_spare_layout():
    """An ``out`` with a wider row stride (nothing outside the n x n block written) and the spare-column layout."""
    import torch

    from infercnvpy_amd import _engine

    n, d = 1100, 143
    X, Zc = E.dist_case(n, d, seed=9, dup=4)
    xd = _gpu(X)
    exp = _exact32(Zc)
    buf = torch.full((n + 3, n + 37), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[:n, :n]
    assert out.stride(0) == n + 37
    _engine.pairwise_sqeuclidean(xd, out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    assert torch.isnan(buf[:, n:]).all() and torch.isnan(buf[n:]).all()
    # a row block into a strided out
    buf.fill_(float("nan"))
    _engine.pairwise_sqeuclidean(xd, out=buf[:200, :n], rows=(1000, 1100))
    np.testing.assert_array_equal(buf[:100, :n].cpu().numpy(), exp[1000:1100])
    assert torch.isnan(buf[:, n:]).all() and torch.isnan(buf[100:]).all()
    sp_out = _engine.pairwise_sqeuclidean(xd, spare=True)
    assert sp_out.shape == (n, n)
    if _engine.has_spare_columns(sp_out):
        assert sp_out.stride(0) == _engine.spare_stride(n)
    np.testing.assert_array_equal(sp_out.cpu().numpy(), exp)


@pytest.mark.parametrize("n", [2500, 3073])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_distance_tiles_exact(n, world):
    """Every rank's super-tiles of a sharded job (icv_pairwise_sqeuclidean_tiles with WardLayout.tile_plan, as
    HipWardSteps.distances calls it), all ranks on one GPU: the direct rows plus the mirror blocks, exchanged and
    unpacked as ward_linkage_sharded does, rebuild the exact matrix."""
    import torch

    from infercnvpy_amd import _engine, _lib, dist

    lib = _lib.load()
    X, Zc = E.dist_case(n, 161, seed=n + world, dup=6)
    xd = _gpu(X)
    exp = _exact32(Zc)
    nan = float("nan")
    layouts = [dist.WardLayout(n, world, r) for r in range(world)]
    local, mirror = [], []
    for L in layouts:
        row0, col0, dir_off, mir_off = L.tile_plan()
        d_local = torch.full((L.rows_padded, L.ld), nan, dtype=torch.float32, device="cuda")
        mir = torch.full((int(L.dest_row0[-1]), L.rows_padded), nan, dtype=torch.float32, device="cuda")
        p = _engine._ptr
        _lib.check(lib.icv_pairwise_sqeuclidean_tiles(
            p(xd), n, xd.shape[1], xd.stride(0), len(row0), row0.ctypes.data, col0.ctypes.data, dir_off.ctypes.data,
            mir_off.ctypes.data, p(d_local), d_local.stride(0), p(mir), mir.stride(0), _engine._stream_ptr(torch)))
        local.append(d_local)
        mirror.append(mir)
    torch.cuda.synchronize()
    for r, L in enumerate(layouts):
        # the direct rows: the super-tiles on and above the diagonal of this rank's super-rows
        for ly, gy in enumerate(L.supers_of[r]):
            r0, r1 = gy * L.S, min(n, (gy + 1) * L.S)
            c0 = gy * L.S
            blk = local[r][ly * L.S:ly * L.S + (r1 - r0), c0:n].cpu().numpy()
            np.testing.assert_array_equal(np.triu(blk, 0)[:, :r1 - r0], np.triu(exp[r0:r1, c0:r1], 0))
            np.testing.assert_array_equal(blk[:, r1 - r0:], exp[r0:r1, r1:])
        # the mirror blocks every rank sent to rank r, unpacked below the diagonal
        lo, hi = int(L.dest_row0[r]), int(L.dest_row0[r + 1])
        recv_from = [mirror[s][lo:hi] for s in range(world)]
        dist._unpack_mirror(L, local[r], recv_from)
    full = torch.empty((n, n), dtype=torch.float32, device="cuda")
    g = np.arange(n)
    own, lrow = layouts[0].row_owner(g), layouts[0].lrow(g)
    for r in range(world):
        sel = np.flatnonzero(own == r)
        full[torch.from_numpy(sel).cuda()] = local[r][torch.from_numpy(lrow[sel]).cuda(), :n]
    np.testing.assert_array_equal(full.cpu().numpy(), exp)


def test_pairwise_output_past_2_31_elements():
    """n = 46 341: the n x n output passes 2^31 elements.  Sampled rows (both ends, both sides of 1024-row
    boundaries, random) are gathered on the GPU and compared with exact rows computed on the host."""
    import torch

    from infercnvpy_amd import _engine

    n, d = 46341, 40
    assert n * n > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < (12 << 30):
        pytest.skip(f"needs ~12 GB of free HBM for the {n} x {n} float32 matrix, {free / 2 ** 30:.1f} GB free")
    X, Zc = E.dist_case(n, d, seed=46341, dup=20)
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([[0, 1, n - 2, n - 1, 1023, 1024, 2047, 2048, 32767, 32768, 45055, 45056,
                                      46079, 46080], rng.integers(0, n, 50)]))
    out = _engine.pairwise_sqeuclidean(_gpu(X))
    got = out[torch.from_numpy(rows).cuda()].cpu().numpy()
    col = out[:, n - 1].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    np.testing.assert_array_equal(got, _exact32(Zc, rows))
    np.testing.assert_array_equal(col, _exact32(Zc, [n - 1])[0])  # the last column = the last row (symmetry)

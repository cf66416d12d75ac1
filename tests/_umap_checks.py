"""What the GPU tests of tl.umap share: the device CSR of a graph, a run of device epochs, and the comparison of ONE
device epoch with the numpy oracle (tests/_umap_oracle.py) from the same snapshot."""
import numpy as np
import scipy.sparse as sp

import _umap_oracle as uo

A, B = uo.A_DEFAULT, uo.B_DEFAULT


def device(g):
    import torch

    g = sp.csr_matrix(g)
    return (torch.from_numpy(g.indptr.astype(np.int64)).cuda(), torch.from_numpy(g.indices.astype(np.int32)).cuda(),
            torch.from_numpy(g.data.astype(np.float32)).cuda())


def gpu_epochs(dev, y, t0, t1, n_epochs, seed, a=A, b=B, **kw):
    import torch

    from infercnvpy_amd import _engine

    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda()
    _engine.umap_epochs(*dev, yd, a=a, b=b, n_epochs=n_epochs, epoch_begin=t0, epoch_end=t1, random_state=seed, **kw)
    return yd.cpu().numpy()


def check_epoch(og, dev, y, t, n_epochs, seed, what, a=A, b=B, **kw):
    """Epoch t on the device against the oracle, both from y; `kw` (gamma, negative_sample_rate, initial_alpha) goes to
    both.  Returns the device's positions."""
    ref, m = uo.epoch(og, y, t, n_epochs=n_epochs, a=a, b=b, seed=seed, **kw)
    got = gpu_epochs(dev, y, t, t + 1, n_epochs, seed, a=a, b=b, **kw)
    if t == 0:
        assert got.tobytes() == y.tobytes(), what
        return got
    tol = uo.tolerance(ref, m)  # derived, not measured: spacing(|ref|) + m_i 2^-32
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), (what, float((err - tol).max()), int((err > tol).sum()))
    assert np.array_equal(got[m == 0], y[m == 0]), what
    return got


def coincident(og, y):
    """Both ends of some entries (and hence the rows of those entries) at the same point: d2 == 0."""
    y = y.copy()
    if len(og.w):
        e = np.arange(0, len(og.w), max(len(og.w) // 50, 1))
        y[og.indices[e]] = y[og.rows[e]]
    y[-1] = y[0]
    return y

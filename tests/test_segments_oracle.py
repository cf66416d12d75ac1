"""The oracle of tl.cnv_segments (tests/_segments_oracle.py) against tables written out by hand, its
round trip on planted call matrices, the consensus rule at its limits, and everything tl.cnv_segments refuses before
it touches the device.  No GPU."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import _segments_oracle as sg
import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# three chromosomes over W = 8: windows [0, 3), [3, 4) (one window) and [4, 8)
EDGES = [0, 3, 4, 8]
HAND_ROWS = [
    [0, 0, 0, 0, 0, 0, 0, 0],          # 0: empty
    [1, 1, 1, 1, 1, 1, 1, 1],          # 1: all gain over three chromosomes: three segments
    [0, -1, 1, 0, 0, 0, 0, 0],         # 2: -1 directly followed by +1: two segments
    [0, 0, 0, 0, 0, 0, -1, -1],        # 3: a run ending at W - 1
    [0, 0, 0, 1, 0, 0, 0, 0],          # 4: the chromosome of one window, alone
    [1, -1, 1, -1, 1, -1, 1, -1],      # 5: alternating: W segments
    [-1, -1, -1, 0, 0, 0, 0, 0],       # 6: exactly one whole chromosome
    [0, 0, -1, -1, -1, 0, 0, 0],       # 7: the same state on both sides of two boundaries: three segments
    [1, 0, 0, 0, 0, 0, 0, 0],          # 8: a run of one window at window 0
    [0, 0, 0, 0, 0, 0, 0, 1],          # 9: a run of one window at W - 1
    [0, 1, 1, 0, -1, -1, 0, 1],        # 10: runs separated by neutral windows
    [-1, -1, -1, -1, -1, -1, -1, 1],   # 11: all loss, the last window gained
]
# (row, start, end, state) in the order of the contract
HAND_SEGMENTS = [
    (1, 0, 3, 1), (1, 3, 4, 1), (1, 4, 8, 1),
    (2, 1, 2, -1), (2, 2, 3, 1),
    (3, 6, 8, -1),
    (4, 3, 4, 1),
    (5, 0, 1, 1), (5, 1, 2, -1), (5, 2, 3, 1), (5, 3, 4, -1), (5, 4, 5, 1), (5, 5, 6, -1), (5, 6, 7, 1), (5, 7, 8, -1),
    (6, 0, 3, -1),
    (7, 2, 3, -1), (7, 3, 4, -1), (7, 4, 5, -1),
    (8, 0, 1, 1),
    (9, 7, 8, 1),
    (10, 1, 3, 1), (10, 4, 6, -1), (10, 7, 8, 1),
    (11, 0, 3, -1), (11, 3, 4, -1), (11, 4, 7, -1), (11, 7, 8, 1),
]
HAND_COUNTS = [0, 3, 2, 1, 1, 8, 1, 3, 1, 1, 3, 4]


def test_hand_written_rows_give_the_hand_written_tables():
    got = sg.segments(np.asarray(HAND_ROWS, dtype=np.int8), EDGES)
    want = np.asarray(HAND_SEGMENTS)
    assert got["counts"].tolist() == HAND_COUNTS and got["counts"].dtype == np.int64
    assert got["offsets"].tolist() == [0] + np.cumsum(HAND_COUNTS).tolist() and got["offsets"].dtype == np.int64
    assert got["row"].tolist() == want[:, 0].tolist() and got["row"].dtype == np.int64
    assert got["start"].tolist() == want[:, 1].tolist() and got["start"].dtype == np.int32
    assert got["end"].tolist() == want[:, 2].tolist() and got["end"].dtype == np.int32
    assert got["state"].tolist() == want[:, 3].tolist() and got["state"].dtype == np.int8


def test_one_chromosome_joins_what_three_split():
    got = sg.segments(np.asarray(HAND_ROWS, dtype=np.int8), [0, 8])
    assert got["counts"].tolist() == [0, 1, 2, 1, 1, 8, 1, 1, 1, 1, 3, 2]


@pytest.mark.parametrize("lengths, n, seed", [([40, 1, 25, 60], 50, 0), ([7], 9, 1), ([1, 1, 1, 5, 16], 30, 2)])
def test_painting_the_segments_gives_the_matrix_back(lengths, n, seed):
    c = so.planted(n, lengths, seed)
    S = c["truth"]
    edges = sg.bounds(c["chr_pos"], S.shape[1])
    got = sg.segments(S, edges)
    assert got["row"].shape[0] == got["offsets"][-1] > 0
    assert np.array_equal(sg.paint(S.shape, got["row"], got["start"], got["end"], got["state"]), S)
    order = np.lexsort((got["start"], got["row"]))
    assert np.array_equal(order, np.arange(order.shape[0]))  # rule 2
    # no segment crosses a chromosome boundary
    chrom = np.searchsorted(edges, got["start"], side="right")
    assert np.array_equal(chrom, np.searchsorted(edges, got["end"] - 1, side="right"))

    codes = np.arange(n) % 4 - 1  # -1: no group; groups 0, 1, 2
    grp = sg.group_segments(S, codes, 3, edges, min_fraction=0.05)
    assert grp["consensus"].any()
    assert np.array_equal(sg.paint((3, S.shape[1]), grp["row"], grp["start"], grp["end"], grp["state"]), grp["consensus"])
    assert grp["n_cells"].tolist() == np.bincount(codes[codes >= 0], minlength=3).tolist()
    assert int(grp["loss"].sum() + grp["gain"].sum()) == int((S[codes >= 0] != 0).sum())
    nd = np.asarray([sg.need(0.05, c) for c in grp["n_cells"]])
    assert (grp["cells_min"] >= nd[grp["row"]]).all() and (grp["support"] >= 0.05).all() and (grp["support"] <= 1).all()
    assert np.array_equal(grp["cells_sum"] >= grp["cells_min"].astype(np.int64) * grp["n_windows"], np.ones_like(grp["row"], bool))


def test_need_is_the_exact_ceiling():
    assert sg.need(0.5, 5) == 3 and sg.need(0.5, 4) == 2 and sg.need(0.5, 1) == 1  # odd n_g rounds up
    assert sg.need(1.0, 7) == 7 and sg.need(1.0, 1) == 1
    assert sg.need(0.5, 0) == 1 and sg.need(1.0, 0) == 1  # a group of no cells needs a vote it cannot get
    assert sg.need(0.1, 3) == 1 and sg.need(1e-9, 1000) == 1
    # exact: 0.1 is a little more than 1/10 as a float, so 10 cells need 2
    assert sg.need(0.1, 10) == 2 and sg.need("1/10", 10) == 1 and sg.need(0.25, 8) == 2 and sg.need(0.25, 9) == 3


def test_consensus_rule_ties_thresholds_and_empty_groups():
    #             window: 0  1  2  3  4  5
    loss = np.asarray([[2, 3, 0, 2, 1, 5],    # group 0: 5 cells, need 3 at min_fraction 0.5
                       [0, 0, 0, 0, 0, 0],    # group 1: no cells
                       [1, 0, 1, 0, 0, 0]], dtype=np.int32)  # group 2: one cell
    gain = np.asarray([[2, 2, 3, 3, 4, 0],
                       [0, 0, 0, 0, 0, 0],
                       [0, 1, 0, 0, 0, 0]], dtype=np.int32)
    n_cells = np.asarray([5, 0, 1])
    got = sg.consensus(loss, gain, n_cells, 0.5)
    assert got.dtype == np.int8
    # tie 2:2 -> 0; 3 losses win; 3 gains win; 3 gains against 2 losses win; 4 gains; 5 losses
    assert got[0].tolist() == [0, -1, 1, 1, 1, -1]
    assert got[1].tolist() == [0] * 6
    assert got[2].tolist() == [-1, 1, -1, 0, 0, 0]
    # min_fraction 1.0: every cell has to agree
    assert sg.consensus(loss, gain, n_cells, 1.0)[0].tolist() == [0, 0, 0, 0, 0, -1]
    # a tie above the threshold stays neutral
    assert sg.consensus(np.asarray([[3]], np.int32), np.asarray([[3]], np.int32), np.asarray([6]), 0.5).tolist() == [[0]]


def test_group_segments_by_hand():
    S = np.asarray([[1, 1, 1, 0, -1, -1],
                    [1, 1, 0, 0, -1, -1],
                    [1, 0, 0, 0, -1, 1],
                    [0, 0, 0, 0, 1, 1]], dtype=np.int8)
    codes = np.asarray([0, 0, 0, -1])
    got = sg.group_segments(S, codes, 2, [0, 2, 6], min_fraction=0.5)  # group 1 has no cells; need_0 = 2
    assert got["gain"].tolist() == [[3, 2, 1, 0, 0, 1], [0] * 6] and got["loss"].tolist() == [[0, 0, 0, 0, 3, 2], [0] * 6]
    assert got["consensus"].tolist() == [[1, 1, 0, 0, -1, -1], [0] * 6]
    assert got["row"].tolist() == [0, 0] and got["start"].tolist() == [0, 4] and got["end"].tolist() == [2, 6]
    assert got["state"].tolist() == [1, -1] and got["cells_min"].tolist() == [2, 2] and got["cells_sum"].tolist() == [5, 5]
    assert got["support"].tolist() == [5 / 6, 5 / 6] and got["n_cells"].tolist() == [3, 0]
    assert got["counts"].tolist() == [2, 0] and got["offsets"].tolist() == [0, 2, 2]


# ---- what tl.cnv_segments refuses without a GPU ---------------------------------------------------------------------------
def _adata(n=4, w=6, x=None, chr_pos=None, obs=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 2), dtype=np.float32), obs=obs)
    ad.obsm["X_cnv_states"] = np.zeros((n, w), dtype=np.int8) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def test_missing_keys_raise_keyerror_with_a_hint():
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(KeyError, match=r"X_other.*Did you run `tl.cnv_states`"):
        cnv.tl.cnv_segments(ad, use_rep="other")
    with pytest.raises(KeyError, match=r"chr_pos.*Did you run `tl.cnv_states`"):
        cnv.tl.cnv_segments(ad, cnv_key="other")
    del ad.uns["cnv"]["chr_pos"]
    with pytest.raises(KeyError, match="chr_pos"):
        cnv.tl.cnv_segments(ad)
    del ad.obsm["X_cnv_states"]
    with pytest.raises(KeyError, match="X_cnv_states"):
        cnv.tl.cnv_segments(ad)


@pytest.mark.parametrize("x, match", [
    (np.zeros((4, 6), dtype=np.float32), "int8"),
    (np.zeros((4, 6), dtype=np.int32), "int8"),
    (np.zeros((4, 6), dtype=np.uint8), "int8"),
    (np.zeros(6, dtype=np.int8), "2-D"),
    (np.zeros((4, 6, 1), dtype=np.int8), "2-D"),
    (np.zeros((0, 6), dtype=np.int8), "empty"),
    (np.zeros((4, 0), dtype=np.int8), "empty"),
])
def test_a_matrix_that_is_not_2d_int8_and_non_empty_raises(x, match):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=match):
        cnv.tl.cnv_segments(_adata(x=x))


def test_a_float_torch_tensor_raises():
    import torch

    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match="int8"):
        cnv.tl.cnv_segments(_adata(x=torch.zeros((4, 6))))


@pytest.mark.parametrize("kw", [
    {"min_fraction": 0}, {"min_fraction": 0.0}, {"min_fraction": -0.5}, {"min_fraction": 1.0000001},
    {"min_fraction": float("nan")}, {"min_fraction": float("inf")}, {"min_fraction": None}, {"min_fraction": "half"},
    {"min_fraction": True},
    {"min_windows": 0}, {"min_windows": -1}, {"min_windows": 1.5}, {"min_windows": None}, {"min_windows": "two"},
    {"min_windows": True}, {"min_windows": float("nan")},
])
def test_bad_parameters_raise_valueerror(kw):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=next(iter(kw))):
        cnv.tl.cnv_segments(_adata(), **kw)
    with pytest.raises(ValueError, match=next(iter(kw))):
        cnv.tl.cnv_segments(_adata(obs=pd.DataFrame({"clone": list("abab")})), "clone", **kw)


def test_unknown_groupby_raises_valueerror():
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match="nothing_here"):
        cnv.tl.cnv_segments(_adata(), "nothing_here")
    with pytest.raises(ValueError, match="tl.leiden"):
        cnv.tl.cnv_segments(_adata(), groupby="cnv_leiden")


@pytest.mark.parametrize("chr_pos, match", [
    ({"chr1": 0, "chr2": 6}, "outside"),
    ({"chr1": 0, "chr2": 4, "chr3": 4}, "same window"),
    ({"chr1": 1, "chr2": 4}, "starts at window 0"),
    ({}, "empty"),
])
def test_chromosome_bounds_keeps_its_errors(chr_pos, match):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError, match=match):
        cnv.tl.cnv_segments(_adata(chr_pos=chr_pos))


def test_windows_beyond_the_states_cap_are_not_refused_by_the_arguments():
    """No row is held in LDS: W above ICV_STATES_MAX_WINDOWS passes every check that needs no device.  The call then
    runs, or stops where it first needs the GPU that is not there."""
    import torch

    import infercnvpy_amd as cnv

    ad = _adata(n=1, w=so.MAX_WINDOWS + 1, chr_pos={"chr1": 0})
    try:
        table = cnv.tl.cnv_segments(ad, inplace=False)
    except RuntimeError as e:
        assert "needs an AMD GPU" in str(e) and not torch.cuda.is_available()
    else:
        assert len(table) == 0


def test_symbols_are_exported_and_declared():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_segments_count", "icv_segments_fill", "icv_state_votes", "icv_state_consensus",
                 "icv_segments_support"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert "cnv_segments" in cnv.tl.__all__


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes

    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first
    bad = _lib.ICV_ERR_INVALID
    assert lib.icv_segments_count(None, 1, 5, one, 1, one, one, None) == bad
    assert lib.icv_segments_count(one, 1, 0, one, 1, one, one, None) == bad       # no windows
    assert lib.icv_segments_count(one, 1, 5, one, 0, one, one, None) == bad       # no chromosome
    assert lib.icv_segments_count(one, 1, 5, one, 6, one, one, None) == bad       # more chromosomes than windows
    assert lib.icv_segments_count(one, -1, 5, one, 1, one, one, None) == bad
    assert lib.icv_segments_count(one, 1, 5, one, 1, None, one, None) == bad
    assert lib.icv_segments_fill(one, 1, 5, one, 1, None, 3, one, one, one, one, None) == bad
    assert lib.icv_segments_fill(one, 1, 5, one, 1, one, -1, one, one, one, one, None) == bad
    assert lib.icv_segments_fill(one, 1, 5, one, 1, one, 3, one, None, one, one, None) == bad
    assert lib.icv_segments_fill(one, 1, 5, one, 1, one, 0, None, None, None, None, None) == _lib.ICV_OK  # nothing to fill
    assert lib.icv_state_votes(None, 1, 5, one, 1, one, 1, one, one, one, None) == bad
    assert lib.icv_state_votes(one, 1, 5, None, 1, one, 1, one, one, one, None) == bad
    assert lib.icv_state_votes(one, 1, 5, one, 1, None, 1, one, one, one, None) == bad
    assert lib.icv_state_votes(one, 1, 5, one, 1, one, 1, None, one, one, None) == bad
    assert lib.icv_state_votes(one, 1, 5, one, -1, one, 1, one, one, one, None) == bad
    assert lib.icv_state_consensus(None, one, one, 1, 5, one, None) == bad
    assert lib.icv_state_consensus(one, one, one, 1, 0, one, None) == bad
    assert lib.icv_state_consensus(None, None, None, 0, 5, None, None) == _lib.ICV_OK  # no groups: nothing runs
    assert lib.icv_segments_support(one, one, one, one, 2, one, one, 1, 5, None, one, None) == bad
    assert lib.icv_segments_support(one, one, one, one, -1, one, one, 1, 5, one, one, None) == bad
    assert lib.icv_segments_support(None, None, None, None, 0, None, None, 1, 5, None, None, None) == _lib.ICV_OK

"""tl.cnv_segments on the GPU equals the oracle of DESIGN.md 4.14 (tests/_segments_oracle.py) byte for byte: every row
geometry, runs at their limits, the votes over one, two and three row blocks, host and device input, and the chain
tl.cnv_states -> tl.cnv_segments."""
import functools

import numpy as np
import pandas as pd
import pytest

import _segments_oracle as sg
import _states_oracle as so

pytestmark = pytest.mark.gpu

TABLE = ("row", "start", "end", "state")


def _adata(S, chr_pos, obs=None, n=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((S.shape[0] if n is None else n, 2), dtype=np.float32), obs=obs)
    ad.obsm["X_cnv_states"] = S
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def random_states(n, lengths, seed):
    """Even rows: runs of 1 .. 40 windows of a random call laid over the row regardless of the chromosomes (so runs
    meet the boundaries); odd rows: the planted truth of tests/_states_oracle.py."""
    rng = np.random.default_rng(seed)
    S = so.planted(n, lengths, seed)["truth"].copy()
    w = S.shape[1]
    for i in range(0, n, 2):
        runs = rng.integers(1, 41, size=w)
        vals = rng.integers(-1, 2, size=w).astype(np.int8)
        S[i] = np.repeat(vals, runs)[:w]
    return S


def layouts(w):
    """Chromosome lengths: one chromosome; min(W, 65) chromosomes; lengths that include 1 at both ends and inside."""
    out = [[w]]
    c = min(w, 65)
    many = [w // c] * c
    many[-1] += w - sum(many)
    out.append(many)
    if w >= 5:
        out.append([1, (w - 3) // 2, 1, w - 3 - (w - 3) // 2, 1])
    return out


def device_tables(S, edges):
    """The unfiltered device tables of rules 1-2 as host arrays."""
    import torch

    from infercnvpy_amd import _engine

    t = S if torch.is_tensor(S) else torch.from_numpy(S).cuda()
    counts, offsets, row, start, end, state, bad = _engine.segments_tables(t, np.asarray(edges, dtype=np.int32))
    assert counts.dtype == torch.int64 and offsets.dtype == torch.int64 and row.dtype == torch.int64
    assert start.dtype == torch.int32 and end.dtype == torch.int32 and state.dtype == torch.int8
    assert int(bad.item()) == 0
    return {"counts": counts.cpu().numpy(), "offsets": offsets.cpu().numpy(), "row": row.cpu().numpy(),
            "start": start.cpu().numpy(), "end": end.cpu().numpy(), "state": state.cpu().numpy()}


def check_rows(S, lengths, label):
    import infercnvpy_amd as cnv

    chr_pos = so.chr_pos_of(lengths)
    edges = sg.bounds(chr_pos, S.shape[1])
    want = sg.segments(S, edges)
    got = device_tables(S, edges)
    print(f"{label}: {S.shape}, {len(lengths)} chromosomes, {want['row'].shape[0]} segments")
    for k in ("counts", "offsets") + TABLE:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (label, k)
    table = cnv.tl.cnv_segments(_adata(S, chr_pos), inplace=False)
    assert list(table.columns) == ["cell", "chromosome", "start", "end", "state", "n_windows"]
    assert table["cell"].dtype == np.int64 and table["start"].dtype == np.int32 and table["end"].dtype == np.int32
    assert table["state"].dtype == np.int8 and table["n_windows"].dtype == np.int32
    for k, col in zip(TABLE, ("cell", "start", "end", "state")):
        assert np.array_equal(table[col].to_numpy(), want[k]), (label, col)
    assert np.array_equal(table["n_windows"].to_numpy(), want["end"] - want["start"])
    names = {v: k for k, v in chr_pos.items()}
    first = np.asarray(edges[:-1])
    assert table["chromosome"].tolist() == [names[int(first[np.searchsorted(first, s, side="right") - 1])]
                                            for s in want["start"]]
    return want


@pytest.mark.parametrize("w", [1, 63, 64, 65, 257, 1801, 4099])
def test_every_row_geometry_equals_the_oracle(w):
    """An odd W puts every second row at an odd address; 1801 and 4099 take two and five steps of 1024 windows."""
    total = 0
    for n in (1, 3, 130):
        for k, lengths in enumerate(layouts(w)):
            S = random_states(n, lengths, 1000 * w + 10 * n + k)
            total += check_rows(S, lengths, f"W={w} n={n} layout={k}")["row"].shape[0]
    assert total > 0


def test_rows_longer_than_the_states_cap():
    w = 20000
    assert w > so.MAX_WINDOWS
    lengths = [9000, 1, 6999, 4000]
    S = random_states(5, lengths, 77)
    S[4] = 1  # one run per chromosome, across every strip
    want = check_rows(S, lengths, "W=20000")
    assert want["counts"][4] == 4


def test_runs_at_their_limits():
    w, cut = 2501, 1300  # three steps of 1024 windows; the odd W moves every row to another alignment
    rows = {
        "full_gain": np.ones(w),
        "all_zero_between_full_rows": np.zeros(w),
        "full_loss": -np.ones(w),
        "alternating": np.where(np.arange(w) % 2 == 0, 1, -1),
        "ends_at_last_window": np.r_[np.zeros(w - 7), np.ones(7)],
        "only_last_window": np.r_[np.zeros(w - 1), [-1]],
        "only_first_window": np.r_[[1], np.zeros(w - 1)],
        "same_state_across_the_boundary": np.r_[np.zeros(cut - 3), -np.ones(6), np.zeros(w - cut - 3)],
        "loss_then_gain": np.r_[np.zeros(100), -np.ones(930), np.ones(930), np.zeros(w - 1960)],
        "neutral_only_at_lane_edges": (np.arange(w) % 16 != 15).astype(int),
        "neutral_only_at_step_edges": (np.arange(w) % 1024 != 0).astype(int),
    }
    S = np.asarray(list(rows.values()), dtype=np.int8)
    names = list(rows)
    one = check_rows(S, [w], "limits, one chromosome")
    counts = dict(zip(names, one["counts"].tolist()))
    assert counts["full_gain"] == counts["full_loss"] == 1 and counts["all_zero_between_full_rows"] == 0
    assert counts["alternating"] == w and counts["loss_then_gain"] == 2 and counts["same_state_across_the_boundary"] == 1
    assert counts["neutral_only_at_lane_edges"] == (w + 15) // 16 and counts["neutral_only_at_step_edges"] == 3
    i = names.index("full_gain")
    assert (one["start"][one["row"] == i].tolist(), one["end"][one["row"] == i].tolist()) == ([0], [w])
    two = check_rows(S, [cut, w - cut], "limits, two chromosomes")
    counts = dict(zip(names, two["counts"].tolist()))
    assert counts["full_gain"] == counts["full_loss"] == 2 and counts["same_state_across_the_boundary"] == 2
    i = names.index("same_state_across_the_boundary")
    assert two["start"][two["row"] == i].tolist() == [cut - 3, cut] and two["end"][two["row"] == i].tolist() == [cut, cut + 3]
    assert two["state"][two["row"] == i].tolist() == [-1, -1]
    i = names.index("ends_at_last_window")
    assert two["end"][two["row"] == i].tolist() == [w]
    check_rows(S, [1] * 64 + [w - 64], "limits, 64 chromosomes of one window")


# ---- groups ----------------------------------------------------------------------------------------------------------------
GROUP_SIZES = {"a": 1024, "b": 0, "c": 1, "d": 2049, "e": 1025}  # sizes at, next to and beyond one and two blocks of 1024 listed rows
GROUP_LENGTHS = [700, 1, 500, 600]  # W = 1801


@functools.lru_cache(maxsize=None)
def group_case():
    """Cells of five clones (one of them without cells) and 50 cells without a label, in shuffled order: each cell has
    its clone's pattern of runs with a fifth of its windows redrawn.  dict(S, labels, codes, chr_pos, want)."""
    rng = np.random.default_rng(5)
    w = sum(GROUP_LENGTHS)
    names = list(GROUP_SIZES)
    codes = np.concatenate([np.full(GROUP_SIZES[k], g) for g, k in enumerate(names)] + [np.full(50, -1)])
    rng.shuffle(codes)
    n = codes.shape[0]
    base = random_states(2 * len(names), GROUP_LENGTHS, 9)[::2]  # one pattern per clone (and the unlabelled cells')
    S = base[codes].copy()  # (code -1 takes the last pattern)
    redraw = rng.random((n, w)) < 0.2
    S[redraw] = rng.integers(-1, 2, size=int(redraw.sum())).astype(np.int8)
    labels = pd.Categorical.from_codes(codes, categories=names)
    chr_pos = so.chr_pos_of(GROUP_LENGTHS)
    want = sg.group_segments(S, codes, len(names), sg.bounds(chr_pos, w), min_fraction=0.5)
    S.setflags(write=False)
    return {"S": S, "labels": labels, "codes": codes, "chr_pos": chr_pos, "want": want, "names": names}


def check_group_result(result, c, want=None, min_windows=1):
    want = c["want"] if want is None else want
    table, consensus, loss, gain = result
    assert consensus.dtype == np.int8 and loss.dtype == np.int32 and gain.dtype == np.int32
    assert np.array_equal(loss, want["loss"]) and np.array_equal(gain, want["gain"])
    assert np.array_equal(consensus, want["consensus"])
    keep = want["n_windows"] >= min_windows
    assert list(table.columns) == ["group", "chromosome", "start", "end", "state", "n_windows", "n_cells", "cells_min",
                                   "support"]
    assert table["group"].tolist() == [c["names"][g] for g in want["row"][keep]]
    for col, k in (("start", "start"), ("end", "end"), ("state", "state"), ("n_windows", "n_windows"),
                   ("cells_min", "cells_min"), ("support", "support")):
        assert table[col].dtype == want[k].dtype and np.array_equal(table[col].to_numpy(), want[k][keep]), col
    assert table["n_cells"].dtype == np.int64 and np.array_equal(table["n_cells"].to_numpy(), want["n_cells"][want["row"][keep]])


def test_votes_consensus_and_group_segments_equal_the_oracle():
    import infercnvpy_amd as cnv

    c = group_case()
    want = c["want"]
    assert want["n_cells"].tolist() == list(GROUP_SIZES.values()) and (c["codes"] == -1).sum() == 50
    assert (want["consensus"] == 1).any() and (want["consensus"] == -1).any() and not want["consensus"][1].any()
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": c["labels"]}))
    result = cnv.tl.cnv_segments(ad, "clone", inplace=False, return_info=True)
    info = result[-1]
    check_group_result(result[:4], c)
    assert info["n_groups"] == 5 and info["n_segments"] == want["row"].shape[0] and set(info["stage_ms"]) == {"votes", "segments"}
    loss, gain = result[2], result[3]
    assert int(loss.sum(dtype=np.int64) + gain.sum(dtype=np.int64)) == int((c["S"][c["codes"] >= 0] != 0).sum())
    assert (want["support"] >= 0.5).all() and (want["support"] <= 1.0).all()
    # a column that is not categorical: groups in order of appearance, the missing label ignored
    plain = np.asarray(c["labels"].astype(object))
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": plain}))
    table, consensus, _, _ = cnv.tl.cnv_segments(ad, "clone", inplace=False)
    codes2, uniques = pd.factorize(plain, use_na_sentinel=True)
    want2 = sg.group_segments(c["S"], codes2, len(uniques), sg.bounds(c["chr_pos"], c["S"].shape[1]))
    assert np.array_equal(consensus, want2["consensus"]) and consensus.shape[0] == 4
    assert table["group"].tolist() == [uniques[g] for g in want2["row"]]
    assert np.array_equal(table["support"].to_numpy(), want2["support"])


@pytest.mark.parametrize("min_fraction", [1.0, 0.1, 1e-6])
def test_other_fractions_equal_the_oracle(min_fraction):
    import infercnvpy_amd as cnv

    c = group_case()
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": c["labels"]}))
    want = sg.group_segments(c["S"], c["codes"], 5, sg.bounds(c["chr_pos"], c["S"].shape[1]), min_fraction=min_fraction)
    check_group_result(cnv.tl.cnv_segments(ad, "clone", inplace=False, min_fraction=min_fraction), c, want)


def test_host_and_device_input_give_the_same_bytes():
    import torch

    import infercnvpy_amd as cnv

    c = group_case()
    obs = pd.DataFrame({"clone": c["labels"]})
    S_dev = torch.from_numpy(c["S"].copy()).cuda()
    before = S_dev.clone()
    ad_h, ad_d = _adata(c["S"], c["chr_pos"], obs=obs), _adata(S_dev, c["chr_pos"], obs=obs)
    host, dev = cnv.tl.cnv_segments(ad_h, inplace=False), cnv.tl.cnv_segments(ad_d, inplace=False)
    assert len(host) > 0 and all(host[k].to_numpy().tobytes() == dev[k].to_numpy().tobytes()
                                 for k in ("cell", "start", "end", "state", "n_windows"))
    assert host["chromosome"].tolist() == dev["chromosome"].tolist()
    host, dev = cnv.tl.cnv_segments(ad_h, "clone", inplace=False), cnv.tl.cnv_segments(ad_d, "clone", inplace=False)
    for a, b in zip(host[1:], dev[1:]):
        assert a.tobytes() == b.tobytes()
    assert host[0].equals(dev[0])
    check_group_result(dev, c)
    assert ad_d.obsm["X_cnv_states"] is S_dev and S_dev.is_cuda and torch.equal(S_dev, before)
    # a view that is not contiguous is read as the matrix it shows
    wide = torch.zeros((S_dev.shape[0], S_dev.shape[1] + 3), dtype=torch.int8, device="cuda")
    wide[:, 3:] = S_dev
    ad_v = _adata(wide[:, 3:], c["chr_pos"], obs=obs)
    check_group_result(cnv.tl.cnv_segments(ad_v, "clone", inplace=False), c)


def test_inplace_writes_the_documented_dict_and_min_windows_drops_short_segments():
    import infercnvpy_amd as cnv

    c = group_case()
    want = c["want"]
    assert (want["n_windows"] < 3).any() and (want["n_windows"] >= 3).any()
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": c["labels"]}))
    assert cnv.tl.cnv_segments(ad, "clone", min_windows=3) is None
    out = ad.uns["cnv_segments"]
    assert set(out) == {"segments", "params", "groups", "n_cells", "consensus", "loss", "gain"}
    check_group_result((out["segments"], out["consensus"], out["loss"], out["gain"]), c, min_windows=3)
    assert out["params"] == {"groupby": "clone", "use_rep": "cnv_states", "min_fraction": 0.5, "min_windows": 3}
    assert list(out["groups"]) == c["names"] and out["n_cells"].tolist() == list(GROUP_SIZES.values())
    assert (out["segments"]["n_windows"] >= 3).all()

    S = c["S"][:200]
    edges = sg.bounds(c["chr_pos"], S.shape[1])
    cells = sg.segments(S, edges)
    keep = (cells["end"] - cells["start"]) >= 3
    assert 0 < keep.sum() < keep.shape[0]
    ad = _adata(S, c["chr_pos"])
    table, info = cnv.tl.cnv_segments(ad, key_added="per_cell", min_windows=3, return_info=True)
    assert set(ad.uns["per_cell"]) == {"segments", "params"} and ad.uns["per_cell"]["segments"] is table
    assert info["n_segments"] == keep.shape[0] and info["n_groups"] == 0 and set(info["stage_ms"]) == {"segments"}
    for col, k in (("cell", "row"), ("start", "start"), ("end", "end"), ("state", "state")):
        assert np.array_equal(table[col].to_numpy(), cells[k][keep])


def test_a_value_of_2_raises_valueerror():
    import torch

    import infercnvpy_amd as cnv

    c = group_case()
    S = c["S"][:300].copy()
    codes = c["codes"][:300]
    S[int(np.flatnonzero(codes >= 0)[-1]), 1234] = 2
    obs = pd.DataFrame({"clone": c["labels"][:300]})
    for x in (S, torch.from_numpy(S).cuda()):
        for groupby in (None, "clone"):
            ad = _adata(x, c["chr_pos"], obs=obs)
            with pytest.raises(ValueError, match="other than -1, 0 and \\+1"):
                cnv.tl.cnv_segments(ad, groupby)
            assert "cnv_segments" not in ad.uns
    S[S == 2] = -128
    with pytest.raises(ValueError, match="other than"):
        cnv.tl.cnv_segments(_adata(S, c["chr_pos"]))


def test_chain_from_cnv_states_finds_the_planted_blocks_of_each_clone():
    """planted777: the clone of a cell is the call planted at window 20 (gain, loss or none), so every cell of the
    "gain" clone carries a planted gain block over that window and the block comes back as a consensus segment of that
    clone.  The state matrix stays on the device from tl.cnv_states to the tables."""
    import torch

    import infercnvpy_amd as cnv

    c = so.case("planted777")
    probe = 20
    labels = np.where(c["truth"][:, probe] > 0, "gain", np.where(c["truth"][:, probe] < 0, "loss", "none"))
    assert min((labels == k).sum() for k in ("gain", "loss", "none")) >= 20
    ad = _adata(None, c["chr_pos"], obs=pd.DataFrame({"clone": labels}), n=777)
    del ad.obsm["X_cnv_states"]
    ad.obsm["X_cnv"] = torch.from_numpy(c["x"].toarray()).cuda()
    cnv.tl.cnv_states(ad)
    states = ad.obsm["X_cnv_states"]
    assert torch.is_tensor(states) and states.is_cuda and states.dtype == torch.int8
    table, consensus, loss, gain = cnv.tl.cnv_segments(ad, "clone", inplace=False)
    assert ad.obsm["X_cnv_states"] is states and states.is_cuda
    assert np.array_equal(states.cpu().numpy(), c["states"])
    codes, uniques = pd.factorize(labels)
    want = sg.group_segments(c["states"], codes, len(uniques), sg.bounds(c["chr_pos"], c["states"].shape[1]))
    assert np.array_equal(consensus, want["consensus"]) and np.array_equal(loss, want["loss"])
    assert np.array_equal(gain, want["gain"]) and np.array_equal(table["support"].to_numpy(), want["support"])
    assert np.array_equal(table["start"].to_numpy(), want["start"]) and np.array_equal(table["end"].to_numpy(), want["end"])
    over = table[(table["start"] <= probe) & (table["end"] > probe)]
    assert sorted(zip(over["group"], over["state"])) == [("gain", 1), ("loss", -1)]
    assert (over["chromosome"] == "chr1").all() and (over["support"] >= 0.5).all() and (table["support"] >= 0.5).all()
    assert (over["cells_min"] * 2 >= over["n_cells"]).all()

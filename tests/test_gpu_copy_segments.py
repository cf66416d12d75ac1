"""tl.cnv_copy_segments on the GPU equals the oracle of DESIGN.md 4.25 (tests/_copy_segments_oracle.py) byte for byte: every
row geometry, runs of levels at their limits, every number of planes of the votes, groups over one, two and three row
blocks, the rules of the consensus level, ``p_neutral`` against the filter, and the chains from the calls to the tables."""
import functools

import numpy as np
import pandas as pd
import pytest

import _copy_posterior_oracle as cpo
import _copy_segments_oracle as cs
import _posterior_oracle as po
import _pseudobulk_oracle as pb
import _segments_oracle as sg

pytestmark = pytest.mark.gpu

CELL_COLUMNS = ["cell", "chromosome", "start", "end", "level", "n_windows"]
GROUP_COLUMNS = ["group", "chromosome", "start", "end", "level", "n_windows", "n_cells", "cells_min", "support",
                 "level_cells_min", "level_support"]


def _adata(S, chr_pos, obs=None, P=None, key="cnv_copy_states", pkey="cnv_copy_posterior", model=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((S.shape[0], 2), dtype=np.float32), obs=obs)
    ad.obsm[f"X_{key}"] = S
    if P is not None:
        ad.obsm[f"X_{pkey}_neutral"] = P
    if model is not None:  # (K, z): what tl.cnv_copy_states leaves
        ad.uns["cnv_copy_states"] = {"params": {"levels": [0.1 * (s - model[1]) for s in range(model[0])],
                                                "neutral": model[1], "sigma": 0.1, "switch_prob": 1e-3}}
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def check_cells(S, edges, P=None, lo=-7, hi=7, label="", **kw):
    """The engine's tables and the public per-cell table equal the oracle; returns the oracle's dict (with p_neutral)."""
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    want = cs.segments(S, edges, lo, hi)
    got = _engine.level_segments_tables(torch.from_numpy(np.array(S)).cuda(), np.asarray(edges, dtype=np.int32), lo, hi)
    assert int(got[6].item()) == 0
    for k, v in zip(("counts", "offsets", "row", "start", "end", "level"), got):
        v = v.cpu().numpy()
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (label, k)
    chr_pos = cs.chr_pos_of_edges(edges)
    table = cnv.tl.cnv_copy_segments(_adata(S, chr_pos, P=P), level_range=(lo, hi), inplace=False, **kw)
    assert list(table.columns) == CELL_COLUMNS + (["p_neutral"] if P is not None else [])
    for col, k, dtype in (("cell", "row", np.int64), ("start", "start", np.int32), ("end", "end", np.int32),
                          ("level", "level", np.int8)):
        assert table[col].dtype == dtype and np.array_equal(table[col].to_numpy(), want[k]), (label, col)
    assert table["n_windows"].dtype == np.int32 and np.array_equal(table["n_windows"].to_numpy(), want["end"] - want["start"])
    names = {v: k for k, v in chr_pos.items()}
    first = np.asarray(edges[:-1])
    assert table["chromosome"].tolist() == [names[int(first[np.searchsorted(first, s, side="right") - 1])]
                                            for s in want["start"]]
    if P is not None:
        want["Q"], want["p_neutral"] = cs.p_neutral(P, want["row"], want["start"], want["end"])
        assert table["p_neutral"].dtype == np.float64
        assert np.array_equal(_bits(table["p_neutral"].to_numpy()), _bits(want["p_neutral"])), label
    print(f"{label}: {S.shape}, {len(edges) - 1} chromosomes, {want['row'].shape[0]} segments")
    return want


# ---- rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 63, 64, 65, 257, 1801, 4099])
def test_every_row_geometry_equals_the_oracle(w):
    """5 rows: an odd W puts the rows at every alignment; 1801 and 4099 take two and five steps of 1024 windows."""
    total = 0
    for k in range(3):
        S = cs.random_levels(5, w, 100 * w + k, p_neutral_run=0.3)
        edges = cs.random_edges(w, 7 * w + k, n_chr=(1, 5, 40)[k])
        P = np.random.default_rng(w + k).random(S.shape)
        total += check_cells(S, edges, P, label=f"W={w} layout={k}")["row"].shape[0]
    assert total > 0 or w == 1


def test_runs_at_their_limits():
    w = 4099
    S = np.zeros((5, w), dtype=np.int8)
    S[0, 10:16], S[0, 16:22] = 1, 2          # a level step between two strips of an aligned row (row 0)
    S[0, 1000:1024], S[0, 1024:1050] = 1, 2  # and between two steps of 1024 windows
    S[1, 1990:2000], S[1, 2000:2010] = 3, 4  # a level step at a chromosome start (in the second layout)
    S[1, 2990:3010] = -2                     # a chromosome start inside a run of one level
    S[2, 5:8] = [1, 2, 1]                    # three runs of one window
    S[2, 100:110], S[2, 110:120] = -7, 7
    S[3] = 5                                 # one run over all windows
    S[4, w - 5:] = -3                        # a run that ends at W - 1
    S[4, 3000:3003] = 6                      # over the chromosomes of one window
    P = np.random.default_rng(1).random(S.shape)
    one = check_cells(S, [0, w], P, label="limits, one chromosome")
    tab = list(zip(one["row"].tolist(), one["start"].tolist(), one["end"].tolist(), one["level"].tolist()))
    assert tab == [(0, 10, 16, 1), (0, 16, 22, 2), (0, 1000, 1024, 1), (0, 1024, 1050, 2), (1, 1990, 2000, 3),
                   (1, 2000, 2010, 4), (1, 2990, 3010, -2), (2, 5, 6, 1), (2, 6, 7, 2), (2, 7, 8, 1), (2, 100, 110, -7),
                   (2, 110, 120, 7), (3, 0, w, 5), (4, 3000, 3003, 6), (4, w - 5, w, -3)]
    more = check_cells(S, [0, 2000, 3000, 3001, 3002, w], P, label="limits, chromosomes of one window")
    tab = list(zip(more["row"].tolist(), more["start"].tolist(), more["end"].tolist(), more["level"].tolist()))
    assert (1, 1990, 2000, 3) in tab and (1, 2000, 2010, 4) in tab
    assert (1, 2990, 3000, -2) in tab and (1, 3000, 3001, -2) in tab and (1, 3002, 3010, -2) in tab
    assert [r for r in tab if r[0] == 3] == [(3, 0, 2000, 5), (3, 2000, 3000, 5), (3, 3000, 3001, 5), (3, 3001, 3002, 5),
                                             (3, 3002, w, 5)]
    assert [r for r in tab if r[0] == 4] == [(4, 3000, 3001, 6), (4, 3001, 3002, 6), (4, 3002, 3003, 6), (4, w - 5, w, -3)]


# ---- the level range -------------------------------------------------------------------------------------------------------
def _group_want(S, codes, n_groups, edges, min_fraction, lo, hi):
    return cs.group_segments(S, codes, n_groups, edges, min_fraction, lo, hi)


def check_groups(result, want, names, min_windows=1):
    table, consensus, loss, gain, counts = result
    assert consensus.dtype == np.int8 and loss.dtype == np.int32 and gain.dtype == np.int32 and counts.dtype == np.int32
    assert counts.shape == want["counts"].shape and np.array_equal(counts, want["counts"])
    assert np.array_equal(loss, want["loss"]) and np.array_equal(gain, want["gain"])
    assert np.array_equal(consensus, want["consensus"])
    keep = want["n_windows"] >= min_windows
    assert list(table.columns) == GROUP_COLUMNS
    assert table["group"].tolist() == [names[g] for g in want["row"][keep]]
    for col in ("start", "end", "level", "n_windows", "cells_min", "level_cells_min"):
        assert table[col].dtype == want[col].dtype and np.array_equal(table[col].to_numpy(), want[col][keep]), col
    for col in ("support", "level_support"):
        assert table[col].dtype == np.float64 and np.array_equal(_bits(table[col].to_numpy()), _bits(want[col][keep])), col
    assert table["n_cells"].dtype == np.int64 and np.array_equal(table["n_cells"].to_numpy(), want["n_cells"][want["row"][keep]])


def _noisy_clones(n, w, n_groups, lo, hi, seed, flip=0.3):
    """(S, codes): every cell has its clone's pattern of level runs with a share ``flip`` of the windows redrawn; codes
    hold -1 (no group) too."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(-1, n_groups, size=n)
    base = cs.random_levels(n_groups + 1, w, seed + 1, lo, hi, p_neutral_run=0.4)
    S = base[codes].copy()
    redraw = rng.random(S.shape) < flip
    S[redraw] = rng.integers(lo, hi + 1, size=int(redraw.sum())).astype(np.int8)
    return S, codes


RANGES = [(0, 0), (0, 1), (-1, 1), (-1, 2), (-2, 2), (-2, 3), (-3, 3), (-3, 4), (-4, 4), (-4, 5), (-5, 5), (-5, 6), (-6, 6),
          (-6, 7), (-7, 7), (0, 7), (-7, 0)]


def test_every_number_of_planes_equals_the_oracle():
    """P = hi - lo + 1 from 1 to 15: every instantiation of the votes kernel, on 131 windows (a tail of three columns)."""
    import infercnvpy_amd as cnv

    assert sorted({hi - lo + 1 for lo, hi in RANGES}) == list(range(1, 16))
    w, names = 131, ["g0", "g1", "g2"]
    edges = [0, 37, 38, 102, w]
    for k, (lo, hi) in enumerate(RANGES):
        S, codes = _noisy_clones(70, w, 3, lo, hi, 300 + k)
        obs = pd.DataFrame({"clone": pd.Categorical.from_codes(codes, categories=names)})
        want = _group_want(S, codes, 3, edges, 0.5, lo, hi)
        ad = _adata(S, cs.chr_pos_of_edges(edges), obs=obs)
        check_groups(cnv.tl.cnv_copy_segments(ad, "clone", level_range=(lo, hi), inplace=False), want, names)
        check_cells(S, edges, lo=lo, hi=hi, label=f"range ({lo}, {hi})")


def test_the_level_range_comes_from_the_argument_then_the_model_then_seven():
    import infercnvpy_amd as cnv

    w, edges = 90, [0, 40, 90]
    chr_pos = cs.chr_pos_of_edges(edges)
    names = ["g0", "g1"]
    for model, rng_ in (((8, 0), (0, 7)), ((8, 7), (-7, 0)), ((6, 2), (-2, 3))):
        lo, hi = rng_
        S, codes = _noisy_clones(40, w, 2, lo, hi, 50 + lo)
        assert S.min() == lo and S.max() == hi
        obs = pd.DataFrame({"clone": pd.Categorical.from_codes(codes, categories=names)})
        want = _group_want(S, codes, 2, edges, 0.5, lo, hi)
        ad = _adata(S, chr_pos, obs=obs, model=model)
        cnv.tl.cnv_copy_segments(ad, "clone")
        out = ad.uns["cnv_copy_segments"]
        assert out["params"]["level_range"] == (lo, hi) and out["levels"] == list(range(lo, hi + 1))
        check_groups((out["segments"], out["consensus"], out["loss"], out["gain"], out["counts"]), want, names)
        # the argument overrides the model; without either the range is (-7, 7)
        cnv.tl.cnv_copy_segments(ad, "clone", level_range=(-7, 7), key_added="wide")
        assert ad.uns["wide"]["counts"].shape == (2, 15, w) and ad.uns["wide"]["params"]["level_range"] == (-7, 7)
        assert np.array_equal(ad.uns["wide"]["counts"][:, lo + 7:hi + 8], want["counts"])
        assert np.array_equal(ad.uns["wide"]["consensus"], want["consensus"])
        plain = _adata(S, chr_pos, obs=obs)
        cnv.tl.cnv_copy_segments(plain, "clone")
        assert plain.uns["cnv_copy_segments"]["params"]["level_range"] == (-7, 7)
        # a level inside [-7, 7] and outside the model's range is refused, for both tables
        for groupby in (None, "clone"):
            for narrow in ((lo + 1, hi) if lo < 0 else (lo, hi - 1), ):
                with pytest.raises(ValueError, match=r"levels outside \["):
                    cnv.tl.cnv_copy_segments(ad, groupby, level_range=narrow)
            other = S.copy()
            other[int(np.flatnonzero(codes >= 0)[-1]), w - 1] = hi + 1 if hi < 7 else lo - 1
            with pytest.raises(ValueError, match=r"levels outside \["):
                cnv.tl.cnv_copy_segments(_adata(other, chr_pos, obs=obs, model=model), groupby)
    for value in (8, -8, -128):
        bad = np.zeros((3, w), dtype=np.int8)
        bad[2, 17] = value
        for groupby in (None, "clone"):
            ad = _adata(bad, chr_pos, obs=pd.DataFrame({"clone": ["a", "a", "b"]}))
            with pytest.raises(ValueError, match=r"levels outside \[-7, 7\]"):
                cnv.tl.cnv_copy_segments(ad, groupby)
            assert "cnv_copy_segments" not in ad.uns
    for level_range in ((-8, 0), (0, 8), (1, 2), (-2, -1), (0.5, 1), "ab", (1, 2, 3)):
        with pytest.raises(ValueError, match="level_range"):
            cnv.tl.cnv_copy_segments(_adata(np.zeros((3, w), dtype=np.int8), chr_pos), level_range=level_range)


# ---- votes -----------------------------------------------------------------------------------------------------------------
GROUP_SIZES = {"a": 1025, "b": 0, "c": 700, "d": 1400}  # sorted rows: a crosses the first block of 1 024, c lies in the
GROUP_LENGTHS = [2000, 1, 1098, 1000]                   # second, d spans the second, third and fourth; W = 4 099


@functools.lru_cache(maxsize=None)
def group_case():
    """Cells of four clones (one without cells) and 30 cells without a label, in shuffled order, levels in [-7, 7]."""
    rng = np.random.default_rng(6)
    w = sum(GROUP_LENGTHS)
    names = list(GROUP_SIZES)
    codes = np.concatenate([np.full(GROUP_SIZES[k], g) for g, k in enumerate(names)] + [np.full(30, -1)])
    rng.shuffle(codes)
    base = cs.random_levels(len(names) + 1, w, 10, p_neutral_run=0.4)
    S = base[codes].copy()
    redraw = rng.random(S.shape) < 0.3
    S[redraw] = rng.integers(-7, 8, size=int(redraw.sum())).astype(np.int8)
    edges = [0, 2000, 2001, 3099, w]
    want = _group_want(S, codes, len(names), edges, 0.5, -7, 7)
    S.setflags(write=False)
    return {"S": S, "codes": codes, "labels": pd.Categorical.from_codes(codes, categories=names), "names": names,
            "edges": edges, "chr_pos": cs.chr_pos_of_edges(edges), "want": want}


def test_votes_over_row_blocks_and_column_tiles_equal_the_oracle():
    import infercnvpy_amd as cnv

    c = group_case()
    want = c["want"]
    assert want["n_cells"].tolist() == list(GROUP_SIZES.values()) and not want["consensus"][1].any()
    assert len(set(np.unique(want["consensus"]).tolist())) > 6 and want["row"].shape[0] > 50
    assert (want["level_cells_min"] < want["cells_min"]).any()
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": c["labels"]}))
    result = cnv.tl.cnv_copy_segments(ad, "clone", inplace=False, return_info=True)
    check_groups(result[:5], want, c["names"])
    info = result[-1]
    assert info["n_groups"] == 4 and info["n_segments"] == want["row"].shape[0] and set(info["stage_ms"]) == {"votes", "segments"}
    counts = result[4]
    assert np.array_equal(counts.sum(axis=1), np.broadcast_to(want["n_cells"][:, None].astype(np.int32), result[2].shape))
    # a column that is not categorical: groups in order of appearance, the missing label ignored
    plain = np.asarray(c["labels"].astype(object))
    codes2, uniques = pd.factorize(plain, use_na_sentinel=True)
    want2 = _group_want(c["S"], codes2, len(uniques), c["edges"], 0.1, -7, 7)
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": plain}))
    check_groups(cnv.tl.cnv_copy_segments(ad, "clone", min_fraction=0.1, inplace=False), want2, list(uniques))


def test_the_pinned_columns_of_the_consensus_rule():
    """Rule 5, one window per row of the issue's table; 8 cells, min_fraction 3 / 8: need = 3."""
    import infercnvpy_amd as cnv

    cols = {"tie_to_the_smaller_magnitude": [1, 1, 1, 2, 2, 2, 0, 0], "the_larger_count": [1, 1, 2, 2, 2, 0, 0, 0],
            "sign_tie": [-1, -1, -1, 2, 2, 2, 0, 0], "gain_exactly_need": [3, 3, 1, 0, 0, 0, 0, -1],
            "gain_at_need_minus_1": [3, 3, 0, 0, 0, 0, 0, -1]}
    S = np.asarray(list(cols.values()), dtype=np.int8).T.copy()
    ad = _adata(S, {"chr1": 0}, obs=pd.DataFrame({"clone": ["g"] * 8}))
    _, consensus, loss, gain, counts = cnv.tl.cnv_copy_segments(ad, "clone", min_fraction=0.375, level_range=(-2, 3),
                                                                inplace=False)
    assert sg.need(0.375, 8) == 3
    assert gain[0].tolist() == [6, 5, 3, 3, 2] and loss[0].tolist() == [0, 0, 3, 1, 1]
    assert consensus[0].tolist() == [1, 2, 0, 3, 0]
    assert counts[0, :, 0].tolist() == [0, 0, 2, 3, 3, 0]
    # the same columns mirrored: losses
    ad = _adata((-S).astype(np.int8), {"chr1": 0}, obs=pd.DataFrame({"clone": ["g"] * 8}))
    _, consensus, loss, gain, _ = cnv.tl.cnv_copy_segments(ad, "clone", min_fraction=0.375, level_range=(-3, 2), inplace=False)
    assert loss[0].tolist() == [6, 5, 3, 3, 2] and gain[0].tolist() == [0, 0, 3, 1, 1]
    assert consensus[0].tolist() == [-1, -2, 0, -3, 0]


# ---- identities with tl.cnv_segments ------------------------------------------------------------------------------------------
def test_three_state_input_gives_the_tables_of_cnv_segments():
    import infercnvpy_amd as cnv

    c = group_case()
    S = np.sign(c["S"][:1500]).astype(np.int8)
    obs = pd.DataFrame({"clone": c["labels"][:1500]})
    ad = _adata(S, c["chr_pos"], obs=obs, key="cnv_states")
    old = cnv.tl.cnv_segments(ad, inplace=False)
    for level_range in ((-1, 1), None):
        new = cnv.tl.cnv_copy_segments(ad, use_rep="cnv_states", level_range=level_range, inplace=False)
        assert len(old) > 1000 and new.rename(columns={"level": "state"}).equals(old)
    old = cnv.tl.cnv_segments(ad, "clone", inplace=False)
    new = cnv.tl.cnv_copy_segments(ad, "clone", use_rep="cnv_states", level_range=(-1, 1), inplace=False)
    for a, b in zip(old[1:], new[1:4]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert new[0].drop(columns=["level_cells_min", "level_support"]).rename(columns={"level": "state"}).equals(old[0])
    assert new[0]["level_cells_min"].equals(new[0]["cells_min"]) and new[0]["level_support"].equals(new[0]["support"])


def test_on_levels_loss_gain_and_the_sign_of_the_consensus_are_those_of_the_sign_plane():
    import infercnvpy_amd as cnv

    c = group_case()
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": c["labels"]}))
    ad.obsm["X_sign"] = np.sign(c["S"]).astype(np.int8)
    for min_fraction in (0.5, 1e-6):
        _, consensus, loss, gain = cnv.tl.cnv_segments(ad, "clone", use_rep="sign", min_fraction=min_fraction, inplace=False)
        _, cons, lo_, ga_, _ = cnv.tl.cnv_copy_segments(ad, "clone", min_fraction=min_fraction, inplace=False)
        assert lo_.tobytes() == loss.tobytes() and ga_.tobytes() == gain.tobytes()
        assert np.sign(cons).astype(np.int8).tobytes() == consensus.tobytes() and (np.abs(cons) > 1).any()


# ---- p_neutral ---------------------------------------------------------------------------------------------------------------
def test_p_neutral_is_the_oracles_on_the_chain_case_and_on_exact_zeros_and_ones():
    c = cpo.chain_case()
    edges = sg.bounds(c["chr_pos"], c["states"].shape[1])
    want = check_cells(np.array(c["states"]), edges, np.array(c["neutral"]), lo=-2, hi=3, label="chain case")
    assert want["p_neutral"].tolist() == [m for _, _, _, m in c["means"]]
    S = np.array([[1, 1, 1, 2, 2, 0, -3, -3, -3, -3], [4, 4, 4, 4, 4, 4, 4, 4, 4, 4]], dtype=np.int8)
    P = np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 0.5, 1.0, 0.0, 1.0, 0.0], [1.0] * 10])
    want = check_cells(S, [0, 10], P, label="zeros and ones")
    assert want["p_neutral"].tolist() == [0.0, 1.0, 0.5, 1.0] and want["Q"][1] == 2 * 2 ** 40


def test_a_run_whose_sum_passes_2_to_53_rounds_once():
    w = 9001 + 64
    rng = np.random.default_rng(3)
    P = np.rint(rng.uniform(0.9, 1.0, size=(2, w)) * cs.TWO40) / cs.TWO40
    S = np.zeros((2, w), dtype=np.int8)
    S[0, 30:9031], S[1, 64:9065] = 3, -1  # (row 1 starts at an odd address; its run ends at W - 1)
    q = np.rint(P * cs.TWO40).astype(np.int64)
    for i, (a, b) in enumerate(((30, 9031), (64, 9065))):
        if int(q[i, a:b].sum()) % 2 == 0:  # an odd sum between 2^53 and 2^54 is no float64
            P[i, a] -= 2.0 ** -40
    want = check_cells(S, [0, w], P, label="9 001 windows")
    assert all(2 ** 53 < t < 2 ** 54 and t % 2 == 1 and int(float(t)) != t for t in want["Q"])


@pytest.mark.parametrize("t", [0.0, 0.2, 0.5, 1.0])
def test_p_neutral_above_t_is_what_the_filter_removes(t):
    import infercnvpy_amd as cnv

    states, p = po.random_calls(40, [150, 1, 182], seed=4)
    rng = np.random.default_rng(9)
    states = (states * rng.integers(1, 4, size=states.shape)).astype(np.int8)  # levels in [-3, 3]: more runs
    chr_pos = {"a": 0, "b": 150, "c": 151}
    seg = cs.segments(states, [0, 150, 151, 333])
    for k, (i, a, b) in enumerate(zip(seg["row"].tolist(), seg["start"].tolist(), seg["end"].tolist())):
        if k % 5 == 0:
            p[i, a:b] = 0.0  # (means of exactly 0 and 1: nothing lies above 1, everything else above 0)
        elif k % 7 == 0:
            p[i, a:b] = 1.0
    ad = _adata(states, chr_pos, P=p)
    table = cnv.tl.cnv_copy_segments(ad, inplace=False)
    filtered, _, _, removed = cnv.tl.cnv_copy_states_filter(ad, max_p_normal=t, inplace=False)
    gone = table["p_neutral"].to_numpy() > t
    print(f"t = {t}: {int(gone.sum())} of {len(table)} runs removed")
    assert int(removed.sum()) == int(gone.sum()) and (t == 1.0 or 0 < gone.sum() < len(table))
    after = cnv.tl.cnv_copy_segments(_adata(filtered, chr_pos, P=p), inplace=False)
    assert after.equals(table[~gone].reset_index(drop=True))


def test_bad_posteriors_and_planes_are_refused_and_a_missing_plane_gives_no_column():
    import torch

    import infercnvpy_amd as cnv

    S = np.array([[0, 2, 2, 2, 0, 0, -1, -1]], dtype=np.int8)
    chr_pos = {"chr1": 0}
    good = np.full(S.shape, 0.25)
    assert cnv.tl.cnv_copy_segments(_adata(S, chr_pos, P=good), inplace=False)["p_neutral"].tolist() == [0.25, 0.25]
    for value in (np.nan, 1.5, -0.25, np.inf):
        for to in (np.asarray, lambda a: torch.from_numpy(a).cuda()):
            bad = good.copy()
            bad[0, 2] = value
            with pytest.raises(ValueError, match="not a number in"):
                cnv.tl.cnv_copy_segments(_adata(S, chr_pos, P=to(bad)))
            outside = good.copy()
            outside[0, 4] = value  # (no run holds window 4: it is not read)
            assert list(cnv.tl.cnv_copy_segments(_adata(S, chr_pos, P=to(outside)), inplace=False)["p_neutral"]) == [0.25, 0.25]
    for plane in (np.zeros((1, 7)), np.zeros((2, 8)), np.zeros(8)):
        with pytest.raises(ValueError, match="has shape"):
            cnv.tl.cnv_copy_segments(_adata(S, chr_pos, P=plane))
    with pytest.raises(ValueError, match="must be float64"):
        cnv.tl.cnv_copy_segments(_adata(S, chr_pos, P=good.astype(np.float32)))
    assert list(cnv.tl.cnv_copy_segments(_adata(S, chr_pos), inplace=False).columns) == CELL_COLUMNS
    assert list(cnv.tl.cnv_copy_segments(_adata(S, chr_pos, P=good), posterior_key=None, inplace=False).columns) == CELL_COLUMNS
    # the group table has no p_neutral, and does not look at the plane
    ad = _adata(S, chr_pos, P=np.zeros((3, 3)), obs=pd.DataFrame({"clone": ["g"]}))
    assert list(cnv.tl.cnv_copy_segments(ad, "clone", inplace=False)[0].columns) == GROUP_COLUMNS


# ---- input, output ------------------------------------------------------------------------------------------------------------
def test_host_and_device_input_give_the_same_tables():
    import torch

    import infercnvpy_amd as cnv

    c = group_case()
    S = np.array(c["S"][:600])
    P = np.random.default_rng(2).random(S.shape)
    obs = pd.DataFrame({"clone": c["labels"][:600]})
    S_dev, P_dev = torch.from_numpy(S).cuda(), torch.from_numpy(P).cuda()
    before = S_dev.clone()
    ad_h, ad_d = _adata(S, c["chr_pos"], obs=obs, P=P), _adata(S_dev, c["chr_pos"], obs=obs, P=P_dev)
    host, dev = cnv.tl.cnv_copy_segments(ad_h, inplace=False), cnv.tl.cnv_copy_segments(ad_d, inplace=False)
    assert len(host) > 1000 and "p_neutral" in host.columns and host.equals(dev)
    mixed = cnv.tl.cnv_copy_segments(_adata(S_dev, c["chr_pos"], P=P), inplace=False)
    assert mixed.equals(host)
    host, dev = cnv.tl.cnv_copy_segments(ad_h, "clone", inplace=False), cnv.tl.cnv_copy_segments(ad_d, "clone", inplace=False)
    for a, b in zip(host[1:], dev[1:]):
        assert isinstance(b, np.ndarray) and a.tobytes() == b.tobytes()
    assert host[0].equals(dev[0]) and len(host[0]) > 10
    assert ad_d.obsm["X_cnv_copy_states"] is S_dev and torch.equal(S_dev, before)
    # a view that is not contiguous is read as the matrix it shows
    wide = torch.zeros((S.shape[0], S.shape[1] + 3), dtype=torch.int8, device="cuda")
    wide[:, 3:] = S_dev
    view = cnv.tl.cnv_copy_segments(_adata(wide[:, 3:], c["chr_pos"], obs=obs), "clone", inplace=False)
    assert view[0].equals(host[0])


def test_inplace_writes_the_documented_dict_and_min_windows_drops_short_segments():
    import infercnvpy_amd as cnv

    c = group_case()
    want = c["want"]
    assert (want["n_windows"] < 3).any() and (want["n_windows"] >= 3).any()
    ad = _adata(c["S"], c["chr_pos"], obs=pd.DataFrame({"clone": c["labels"]}))
    assert cnv.tl.cnv_copy_segments(ad, "clone", min_windows=3) is None
    out = ad.uns["cnv_copy_segments"]
    assert set(out) == {"segments", "params", "groups", "n_cells", "consensus", "levels", "counts", "loss", "gain"}
    check_groups((out["segments"], out["consensus"], out["loss"], out["gain"], out["counts"]), want, c["names"], min_windows=3)
    assert out["params"] == {"groupby": "clone", "use_rep": "cnv_copy_states", "posterior_key": "cnv_copy_posterior",
                             "level_range": (-7, 7), "min_fraction": 0.5, "min_windows": 3}
    assert list(out["groups"]) == c["names"] and out["n_cells"].tolist() == list(GROUP_SIZES.values())
    assert out["levels"] == list(range(-7, 8)) and (out["segments"]["n_windows"] >= 3).all()

    S = np.array(c["S"][:100])
    P = np.random.default_rng(4).random(S.shape)
    cells = cs.segments(S, c["edges"])
    _, mean = cs.p_neutral(P, cells["row"], cells["start"], cells["end"])
    keep = (cells["end"] - cells["start"]) >= 3
    assert 0 < keep.sum() < keep.shape[0]
    ad = _adata(S, c["chr_pos"], P=P)
    table, info = cnv.tl.cnv_copy_segments(ad, key_added="per_cell", min_windows=3, return_info=True)
    assert set(ad.uns["per_cell"]) == {"segments", "params"} and ad.uns["per_cell"]["segments"] is table
    assert info["n_segments"] == keep.shape[0] and info["n_groups"] == 0 and set(info["stage_ms"]) == {"segments", "psum"}
    for col, k in (("cell", "row"), ("start", "start"), ("end", "end"), ("level", "level")):
        assert np.array_equal(table[col].to_numpy(), cells[k][keep])
    assert np.array_equal(_bits(table["p_neutral"].to_numpy()), _bits(mean[keep]))


def test_the_three_state_pair_gives_the_tables_of_cnv_segments_with_p_neutral():
    import infercnvpy_amd as cnv

    c = po.chain_case()
    ad = _adata(np.array(c["states"]), c["chr_pos"], P=np.array(c["neutral"]), key="cnv_states", pkey="cnv_posterior")
    table = cnv.tl.cnv_copy_segments(ad, use_rep="cnv_states", posterior_key="cnv_posterior", inplace=False)
    old = cnv.tl.cnv_segments(ad, inplace=False)
    assert len(old) > 10 and table.drop(columns=["p_neutral"]).rename(columns={"level": "state"}).equals(old)
    seg = cs.segments(c["states"], sg.bounds(c["chr_pos"], c["states"].shape[1]), -1, 1)
    _, want = cs.p_neutral(c["neutral"], seg["row"], seg["start"], seg["end"])
    assert np.array_equal(_bits(table["p_neutral"].to_numpy()), _bits(want))


# ---- the chains ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted_adata(seed):
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    c = cs.planted_clones(seed, 0.15)
    ad = SimpleAnnData(np.zeros((c["x"].shape[0], 2), dtype=np.float32), obs=pd.DataFrame({"clone": c["labels"]}))
    ad.obsm["X_cnv"] = c["x"]
    ad.uns["cnv"] = {"chr_pos": dict(c["chr_pos"])}
    cnv.tl.cnv_copy_states(ad, **c["kwargs"])
    cnv.tl.cnv_copy_posteriors(ad)
    return c, ad


@pytest.mark.parametrize("seed", range(5))
def test_chain_from_the_calls_gives_the_seven_planted_level_segments_of_the_clones(seed):
    import infercnvpy_amd as cnv

    c, ad = _planted_adata(seed)
    table, consensus, _, _, counts = cnv.tl.cnv_copy_segments(ad, "clone", inplace=False)
    assert counts.shape == (3, 6, 130)  # the range (-2, 3) of the model tl.cnv_copy_states left
    assert np.array_equal(consensus, c["clone_truth"])
    got = list(zip(table["group"], table["start"], table["end"], table["level"]))
    assert got == [(f"clone{g}", a, b, v) for g, a, b, v in cs.PLANTED_SEGMENTS]
    assert (table["level_support"] > 0.5).all() and (table["level_support"] <= table["support"]).all()
    sign = cnv.tl.cnv_segments(ad, "clone", use_rep="cnv_copy_states_sign", inplace=False)[0]
    assert len(table) == 7 and len(sign) == cs.PLANTED_SIGN_SEGMENTS == 4
    cells = cnv.tl.cnv_copy_segments(ad, inplace=False)
    assert "p_neutral" in cells.columns and len(cells) >= 7 * 16


@pytest.mark.parametrize("seed", range(5))
def test_chain_over_the_clone_profiles_gives_a_probability_per_clone_segment(seed):
    """tl.cnv_pseudobulk -> tl.cnv_copy_states -> tl.cnv_copy_posteriors -> tl.cnv_copy_segments on the clones.  The CPU
    oracle chain (``_pseudobulk_oracle.profiles``, ``_copy_states_oracle``, ``_copy_posterior_oracle``, this oracle) gives,
    for each of the seeds 0-4, exactly the 7 planted segments with their levels, and the largest ``p_neutral`` of a
    segment is 0.0122, 0.0270, 0.0291, 0.0132 and 0.0158: every clone segment is called with P(neutral) below 0.03.
    The device chain must give the oracle chain's table, ``p_neutral`` bit for bit."""
    import scipy.sparse as sp

    import _copy_states_oracle as co
    import infercnvpy_amd as cnv

    c, ad = _planted_adata(seed)
    clones = cnv.tl.cnv_pseudobulk(ad, "clone")
    cnv.tl.cnv_copy_states(clones, **c["kwargs"])
    cnv.tl.cnv_copy_posteriors(clones)
    table = cnv.tl.cnv_copy_segments(clones, inplace=False)

    mean = pb.profiles(sp.csr_matrix(c["x"]), c["codes"], 3)["mean"]
    states, _, _, params = co.cnv_copy_states(mean, c["chr_pos"], **c["kwargs"])
    planes, _ = cpo.cnv_copy_posteriors(mean, c["chr_pos"], **c["kwargs"])
    seg = cs.segments(states, sg.bounds(c["chr_pos"], 130), *cs.PLANTED_RANGE)
    _, want = cs.p_neutral(planes[params["neutral"]], seg["row"], seg["start"], seg["end"])
    print(f"seed {seed}: p_neutral of the clone segments {want.tolist()}")
    assert list(zip(seg["row"].tolist(), seg["start"].tolist(), seg["end"].tolist(), seg["level"].tolist())) == \
        [tuple(r) for r in cs.PLANTED_SEGMENTS]
    assert want.max() < 0.03
    assert list(zip(table["cell"], table["start"], table["end"], table["level"])) == [tuple(r) for r in cs.PLANTED_SEGMENTS]
    assert np.array_equal(_bits(table["p_neutral"].to_numpy()), _bits(want))

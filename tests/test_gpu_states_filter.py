"""tl.cnv_states_filter on the GPU equals the oracle of DESIGN.md 4.15 (tests/_posterior_oracle.py) byte for byte: the
crafted verdicts, many runs per row, a run longer than any LDS row, unaligned rows, host and device inputs, the bad-value
flag, and the whole chain from tl.cnv_states to the segment table."""
import numpy as np
import pytest

import _posterior_oracle as po
import _segments_oracle as sg
import _states_oracle as so

pytestmark = pytest.mark.gpu


def _adata(states, p, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((states.shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv_states"] = states
    ad.obsm["X_cnv_posterior_neutral"] = p
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _run(states, p, chr_pos, **kw):
    import infercnvpy_amd as cnv

    return cnv.tl.cnv_states_filter(_adata(states, p, chr_pos), inplace=False, **kw)


def _check(states, p, chr_pos, max_p_normal=0.5):
    want, want_fraction, want_removed = po.states_filter(states, p, chr_pos, max_p_normal)
    got, fraction, removed = _run(states, p, chr_pos, max_p_normal=max_p_normal)
    assert isinstance(got, np.ndarray) and got.dtype == np.int8 and got.shape == states.shape
    assert fraction.dtype == np.float64 and removed.dtype == np.int32
    print(f"{states.shape}: {int((got != want).sum())} bytes differ from the oracle, {int(want_removed.sum())} runs removed")
    assert np.array_equal(got, want)
    assert np.array_equal(fraction, want_fraction)
    assert np.array_equal(removed, want_removed)
    return got, removed


@pytest.mark.parametrize("name", list(po.crafted_filter_cases()))
def test_crafted_verdicts(name):
    c = po.crafted_filter_cases()[name]
    got, _ = _check(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])
    assert np.array_equal(got, c["want"])


# ---- the kernel's step boundaries and integer rules ("limits pinned") -------------------------------------------
@pytest.mark.parametrize("neighbourhood", po.SWEEP_NEIGHBOURHOODS)
def test_runs_that_start_end_or_stay_open_at_every_step_boundary(neighbourhood):
    """Every run [s, e) around the lanes 0 and 63 of the 64-window steps, alone, behind a run of the other sign and in
    front of a same-sign run of the next chromosome; the run's integer sum is 0 or 1 above L 2^39, so one window lost or
    counted twice flips the verdict (tests/test_posterior_oracle.py measures it)."""
    removed = 0
    for c in po.sweep_cases(neighbourhood):
        removed += int(_check(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])[1].sum())
    assert removed > 50


def test_half_integer_posteriors_round_half_to_even():
    c = po.half_integer_case()
    got, removed = _check(c["states"], c["p"], c["chr_pos"], c["max_p_normal"])
    assert removed.tolist() == [0, 0, 7] and np.array_equal(got[0], c["states"][0])


def test_sums_above_2_to_53_are_converted_with_one_rounding():
    c = po.big_sum_case()
    assert c["states"].shape[1] == po.BIG_W > po.MAX_WINDOWS
    for i, mean in enumerate(c["means"]):
        got, removed = _check(c["states"], c["p"], c["chr_pos"], mean)
        assert got[i].any() and removed[i] == 0
        got, removed = _check(c["states"], c["p"], c["chr_pos"], float(np.nextafter(mean, 0.0)))
        assert not got[i].any() and removed[i] == 1


def test_thresholds_at_a_runs_own_mean_and_its_float64_neighbours():
    verdicts = []
    for c in po.own_mean_cases():
        verdicts.append(tuple(int(_check(c["states"], c["p"], c["chr_pos"], thr)[1][0]) for thr in c["thresholds"]))
    assert set(verdicts) == {(1, 0, 0)}


def test_more_than_64_runs_in_a_row():
    rng = np.random.default_rng(5)
    w = 431
    states = np.zeros((3, w), dtype=np.int8)
    states[0, ::2] = 1                                    # 216 runs of one window
    states[1] = np.where(np.arange(w) % 3 == 2, 0, np.where(np.arange(w) % 6 < 3, 1, -1))  # runs of two
    states[2] = np.where(np.arange(w) % 2 == 0, 1, -1)    # 431 runs without a neutral window between them
    p = rng.random((3, w))
    pos = {"a": 0, "b": 64, "c": 129, "d": 300}
    _, removed = _check(states, p, pos)
    assert removed.min() > 30
    assert len(po.runs(states[0], so.bounds(pos, w))) > 64


def test_a_run_of_5000_windows_has_no_cap():
    w = 5003
    assert w > po.MAX_WINDOWS
    states = np.zeros((4, w), dtype=np.int8)
    states[:, 2:5002] = 1
    states[2, 2:5002] = -1
    p = np.full((4, w), 0.5)
    p[1, 77] = 0.5 + 2.0 ** -20      # one window tips a run of 5 000
    p[2, 5001] = 0.5 - 2.0 ** -20
    p[3, 2:5002] = np.random.default_rng(1).random(5000)
    got, removed = _check(states, p, {"chr1": 0})
    assert removed.tolist()[:3] == [0, 1, 0] and not got[1].any() and got[0].any()
    _check(states, p, {"chr1": 0, "chr2": 2500, "chr3": 2501})


@pytest.mark.parametrize("lengths", [[1], [63], [64, 1], [65, 64, 63], [129, 2, 700], list(po.LENGTHS_1802)])
def test_random_calls_on_odd_widths(lengths):
    """Rows are W bytes apart: with an odd W every row start has another alignment."""
    states, p = po.random_calls(37, lengths, seed=sum(lengths))
    for thr in (0.5, 0.0, 1.0):
        _check(states, p, so.chr_pos_of(lengths), thr)


def test_empty_and_all_neutral_rows():
    states, p = po.random_calls(9, [50, 51], seed=3)
    states = states.copy()
    states[[0, 4, 8]] = 0
    got, removed = _check(states, p, {"a": 0, "b": 50})
    assert not got[[0, 4, 8]].any() and not removed[[0, 4, 8]].any()
    _check(np.zeros((5, 33), dtype=np.int8), np.ones((5, 33)), {"a": 0})


def test_host_and_device_inputs_give_the_same_bytes():
    import torch

    states, p = po.random_calls(60, [40, 1, 86], seed=8)
    pos = so.chr_pos_of([40, 1, 86])
    want = po.states_filter(states, p, pos)
    for s_in, p_in in ((states, p), (torch.from_numpy(states).cuda(), torch.from_numpy(p).cuda()),
                       (torch.from_numpy(states).cuda(), p), (states, torch.from_numpy(p).cuda())):
        got = _run(s_in, p_in, pos)
        on_device = torch.is_tensor(s_in) or torch.is_tensor(p_in)
        for v, ref in zip(got, want):
            assert torch.is_tensor(v) == on_device
            if on_device:
                assert v.is_cuda
                v = v.cpu().numpy()
            assert v.dtype == ref.dtype and np.array_equal(v, ref)


def test_inplace_writes_obsm_obs_and_uns():
    import torch

    import infercnvpy_amd as cnv

    states, p = po.random_calls(12, [30, 31], seed=2)
    pos = {"a": 0, "b": 30}
    want, want_fraction, want_removed = po.states_filter(states, p, pos, 0.25)
    for s_in in (states, torch.from_numpy(states).cuda()):
        ad = _adata(s_in, p, pos)
        assert cnv.tl.cnv_states_filter(ad, max_p_normal=0.25) is None
        out = ad.obsm["X_cnv_states_filtered"]
        assert torch.is_tensor(out) == torch.is_tensor(s_in)
        assert np.array_equal(out.cpu().numpy() if torch.is_tensor(out) else out, want)
        assert np.array_equal(ad.obs["cnv_states_filtered_fraction"].to_numpy(), want_fraction)
        assert np.array_equal(ad.obs["cnv_states_filtered_removed"].to_numpy(), want_removed)
        assert ad.obs["cnv_states_filtered_removed"].to_numpy().dtype == np.int32
        assert ad.uns["cnv_states_filtered"]["params"]["max_p_normal"] == 0.25


@pytest.mark.parametrize("bad", [1.5, np.nan, -0.5, np.inf])
def test_a_bad_posterior_raises(bad):
    states, p = po.random_calls(6, [70], seed=4)
    p = p.copy()
    p[3, 69] = bad
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        _run(states, p, {"a": 0})
    neutral = np.zeros_like(states)  # also at a window that belongs to no run
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        _run(neutral, p, {"a": 0})


def test_a_state_of_2_raises():
    states, p = po.random_calls(6, [70], seed=4)
    states = states.copy()
    states[5, 0] = 2
    with pytest.raises(ValueError, match="-1, 0 and"):
        _run(states, p, {"a": 0})


def test_the_chain_from_calls_to_the_filtered_segment_table():
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    c = po.chain_case()
    ad = SimpleAnnData(np.zeros((c["x"].shape[0], 2), dtype=np.float32))
    ad.obsm["X_cnv"] = c["x"]
    ad.uns["cnv"] = {"chr_pos": dict(c["chr_pos"])}
    cnv.tl.cnv_states(ad)
    cnv.tl.cnv_posteriors(ad)
    cnv.tl.cnv_states_filter(ad, max_p_normal=po.CHAIN_MAX_P_NORMAL)
    assert np.array_equal(ad.obsm["X_cnv_states"], c["states"])
    assert np.array_equal(ad.obsm["X_cnv_posterior_neutral"], c["neutral"])
    assert np.array_equal(ad.obsm["X_cnv_states_filtered"], c["filtered"])
    assert np.array_equal(ad.obs["cnv_states_filtered_removed"].to_numpy(), c["removed"])
    plain = cnv.tl.cnv_segments(ad, inplace=False)
    table = cnv.tl.cnv_segments(ad, use_rep="cnv_states_filtered", inplace=False)
    edges = so.bounds(c["chr_pos"], c["states"].shape[1])
    want = sg.segments(c["filtered"], edges)
    for column, key in (("cell", "row"), ("start", "start"), ("end", "end"), ("state", "state")):
        assert np.array_equal(table[column].to_numpy(), want[key]), column
    print(f"{len(plain)} segments, {len(table)} after the filter")
    assert len(table) < len(plain) and len(plain) - len(table) == int(c["removed"].sum())
    total, kept = po.planted_segments_kept(c["truth"], ad.obsm["X_cnv_states_filtered"], edges)
    assert total > 1000 and kept == total

"""Numpy / pure-Python oracle of tl.cnv_copy_segments: plain loops over integers, and the builders of
its test cases.

``S`` is the int8 ``n x W`` matrix of copy-number levels (0 neutral, ``-d`` / ``+d`` a loss / gain of distance d), ``edges``
the sorted chromosome starts followed by ``W``.

1. Level range: ``lo <= 0 <= hi`` with ``-7 <= lo`` and ``hi <= 7``; a value outside ``[lo, hi]`` is an error.
2. Runs.  Window t of row i *starts* a run iff ``S[i,t] != 0`` and (t is a chromosome start or ``S[i,t-1] != S[i,t]``); it
   *ends* one iff ``S[i,t] != 0`` and (``t+1 == W`` or t+1 is a chromosome start or ``S[i,t+1] != S[i,t]``): ``+1 +1 +2`` is
   two runs.  Segments are ordered by (row, start).
3. ``p_neutral``: ``q_t = int64(rint(P[i,t] 2^40))``, ``Q`` = the integer sum of q_t over the run,
   ``p_neutral = float(Q) / (float(n_windows) 2^40)``: the mean that ``_copy_posterior_oracle.copy_states_filter`` forms.
4. Votes: ``counts[g, p, w]`` (int32, P = hi - lo + 1) = the cells of group g with level ``lo + p`` at window w (the neutral
   plane included); ``loss[g,w]`` / ``gain[g,w]`` = the sums of the planes with a level < 0 / > 0.
5. Consensus: the sign by rule 5 of ``_segments_oracle`` (``need_g = max(1, ceil(Fraction(min_fraction) n_g))``; ``+`` iff
   ``gain >= need_g`` and ``gain > loss``; ``-`` iff ``loss >= need_g`` and ``loss > gain``; else 0); the magnitude is the
   d in 1 .. (hi or -lo) with the largest ``counts`` of level ``sign d``, the smallest such d on a tie.
6. Group segments: rule 2 on the consensus.  ``cells_min`` / ``cells_sum`` = the minimum / the int64 sum over the segment's
   windows of the cells that carry its *sign* (``loss`` / ``gain``); ``level_cells_min`` / ``level_cells_sum`` the same of
   the cells that carry exactly its *level* (``counts``); ``support`` and ``level_support`` = sum / (n_windows n_g), one
   float64 division each.
"""
import numpy as np

import _copy_states_oracle as co
import _segments_oracle as sg
import _states_oracle as so

MAX_LEVEL = 7
TWO40 = 1099511627776.0


def check_range(lo, hi):
    lo, hi = int(lo), int(hi)
    if not -MAX_LEVEL <= lo <= 0 <= hi <= MAX_LEVEL:
        raise ValueError(f"level range ({lo}, {hi}) must satisfy -7 <= lo <= 0 <= hi <= 7")
    return lo, hi


def check_levels(S, lo, hi):
    S = np.asarray(S)
    if ((S < lo) | (S > hi)).any():
        raise ValueError(f"a level outside [{lo}, {hi}]")


def segments(S, edges, lo=-MAX_LEVEL, hi=MAX_LEVEL):
    """Rules 1-2: dict(counts int64 n, offsets int64 n + 1, row int64, start int32, end int32, level int8)."""
    lo, hi = check_range(lo, hi)
    check_levels(S, lo, hi)
    out = sg.segments(S, edges)  # (its rule 1 compares neighbours for equality: it is rule 2 here)
    out["level"] = out.pop("state")
    return out


def p_neutral(P, row, start, end):
    """Rule 3: (Q as a list of Python integers, p_neutral float64) of the given segments."""
    P = np.asarray(P, dtype=np.float64)
    if not ((P >= 0.0) & (P <= 1.0)).all():
        raise ValueError("a posterior that is not a number in [0, 1]")
    q = np.rint(P * TWO40).astype(np.int64)
    sums = [sum(q[i, a:b].tolist()) for i, a, b in zip(np.asarray(row).tolist(), np.asarray(start).tolist(),
                                                      np.asarray(end).tolist())]
    mean = np.asarray([float(t) / (float(b - a) * TWO40) for t, a, b in
                       zip(sums, np.asarray(start).tolist(), np.asarray(end).tolist())], dtype=np.float64)
    return sums, mean.reshape(len(sums))


def votes(S, codes, n_groups, lo=-MAX_LEVEL, hi=MAX_LEVEL):
    """Rule 4: (counts int32 G x P x W, loss int32 G x W, gain int32 G x W, n_cells int64 G); a code of -1 is no group."""
    lo, hi = check_range(lo, hi)
    S = np.asarray(S)
    n, w = S.shape
    counts = np.zeros((n_groups, hi - lo + 1, w), dtype=np.int32)
    n_cells = np.zeros(n_groups, dtype=np.int64)
    for i in range(n):
        g = int(codes[i])
        if g < 0:
            continue
        check_levels(S[i], lo, hi)
        n_cells[g] += 1
        for p in range(hi - lo + 1):
            counts[g, p] += S[i] == lo + p
    loss = counts[:, :-lo].sum(axis=1, dtype=np.int32).reshape(n_groups, w)
    gain = counts[:, 1 - lo:].sum(axis=1, dtype=np.int32).reshape(n_groups, w)
    return counts, loss, gain, n_cells


def consensus(counts, loss, gain, n_cells, min_fraction, lo, hi):
    """Rule 5: int8 G x W levels."""
    out = np.zeros(loss.shape, dtype=np.int8)
    for g in range(loss.shape[0]):
        nd = sg.need(min_fraction, n_cells[g])
        for t in range(loss.shape[1]):
            lo_n, ga_n = int(loss[g, t]), int(gain[g, t])
            sign = 1 if ga_n >= nd and ga_n > lo_n else -1 if lo_n >= nd and lo_n > ga_n else 0
            if sign == 0:
                continue
            best, most = 0, -1
            for d in range(1, (hi if sign > 0 else -lo) + 1):
                c = int(counts[g, sign * d - lo, t])
                if c > most:
                    best, most = d, c
            out[g, t] = sign * best
    return out


def group_segments(S, codes, n_groups, edges, min_fraction=0.5, lo=-MAX_LEVEL, hi=MAX_LEVEL):
    """Rules 4-6: the dict of :func:`segments` for the consensus matrix (``row`` is the group) plus counts, loss, gain,
    n_cells, consensus, cells_min / level_cells_min int32, cells_sum / level_cells_sum int64, n_windows int32, support /
    level_support float64."""
    counts, loss, gain, n_cells = votes(S, codes, n_groups, lo, hi)
    cons = consensus(counts, loss, gain, n_cells, min_fraction, lo, hi)
    w = np.asarray(S).shape[1]
    out = segments(cons if n_groups else np.zeros((0, w), dtype=np.int8), edges, lo, hi)
    cmin, csum, lmin, lsum = [], [], [], []
    for g, a, b, s in zip(out["row"].tolist(), out["start"].tolist(), out["end"].tolist(), out["level"].tolist()):
        v = (gain if s > 0 else loss)[g, a:b].tolist()
        u = counts[g, s - lo, a:b].tolist()
        cmin.append(min(v)), csum.append(sum(v)), lmin.append(min(u)), lsum.append(sum(u))
    out.update(counts=counts, loss=loss, gain=gain, n_cells=n_cells, consensus=cons,
               cells_min=np.asarray(cmin, dtype=np.int32).reshape(-1), cells_sum=np.asarray(csum, dtype=np.int64).reshape(-1),
               level_cells_min=np.asarray(lmin, dtype=np.int32).reshape(-1),
               level_cells_sum=np.asarray(lsum, dtype=np.int64).reshape(-1))
    out["n_windows"] = (out["end"] - out["start"]).astype(np.int32)
    sizes = [int(k) * int(n_cells[g]) for k, g in zip(out["n_windows"].tolist(), out["row"].tolist())]
    out["support"] = np.asarray([float(c) / float(d) for c, d in zip(csum, sizes)], dtype=np.float64).reshape(-1)
    out["level_support"] = np.asarray([float(c) / float(d) for c, d in zip(lsum, sizes)], dtype=np.float64).reshape(-1)
    return out


def brute_segments(S, edges):
    """Rule 2 by another route: every window gets the number of its chromosome, and a run is grown window by window
    while (chromosome, level) stays the same.  [(row, start, end, level)]."""
    S = np.asarray(S)
    n, w = S.shape
    chrom = np.zeros(w, dtype=np.int64)
    for e in edges[1:-1]:
        chrom[int(e):] += 1
    out = []
    for i in range(n):
        open_run = None  # [start, level, chromosome]
        for t in range(w):
            v, c = int(S[i, t]), int(chrom[t])
            if open_run is not None and (v != open_run[1] or c != open_run[2]):
                out.append((i, open_run[0], t, open_run[1]))
                open_run = None
            if open_run is None and v != 0:
                open_run = [t, v, c]
        if open_run is not None:
            out.append((i, open_run[0], w, open_run[1]))
    return out


# ---- case builders ---------------------------------------------------------------------------------------------------------
def random_levels(n, w, seed, lo=-MAX_LEVEL, hi=MAX_LEVEL, p_neutral_run=0.5):
    """Rows of runs of 1 .. 40 windows: a run is neutral with probability ``p_neutral_run``, else a level drawn from
    lo .. hi (neighbour runs may draw the same level and fuse)."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n, w), dtype=np.int8)
    for i in range(n):
        runs = rng.integers(1, 41, size=w)
        vals = rng.integers(lo, hi + 1, size=w)
        vals[rng.random(w) < p_neutral_run] = 0
        S[i] = np.repeat(vals, runs)[:w].astype(np.int8)
    return S


def random_edges(w, seed, n_chr=None):
    """Sorted chromosome starts (0 among them) followed by w; the starts are drawn at random windows and, where there is
    room, two of them are adjacent (a chromosome of one window)."""
    rng = np.random.default_rng(seed)
    k = min(w, 1 + int(rng.integers(0, 8))) if n_chr is None else min(w, n_chr)
    starts = {0} | set(int(v) for v in rng.choice(w, size=k - 1, replace=False)) if k > 1 else {0}
    if w >= 3:
        t = int(rng.integers(1, w - 1))
        starts |= {t, t + 1}
    return sorted(starts) + [int(w)]


def chr_pos_of_edges(edges):
    """{"chr1": start, ...} of :func:`random_edges`' list, inserted in shuffled order."""
    starts = [int(e) for e in edges[:-1]]
    order = list(range(len(starts)))
    order = order[1::2] + order[0::2]
    return {f"chr{c + 1}": starts[c] for c in order}


PLANTED_LENGTHS = (60, 1, 40, 29)
PLANTED_CLONE_CELLS = 16
PLANTED_STEP = 0.3
# (clone, first window, last window exclusive, level)
PLANTED_SEGMENTS = ((0, 10, 22, 1), (0, 22, 34, 2), (1, 70, 80, -1), (1, 80, 90, -2), (2, 30, 42, 2), (2, 105, 113, 3),
                    (2, 113, 121, 1))
PLANTED_SIGN_SEGMENTS = 4  # [10, 34) +, [70, 90) -, [30, 42) +, [105, 121) +
PLANTED_KWARGS = {"levels": (-0.6, -0.3, 0.0, 0.3, 0.6, 0.9), "sigma": 0.15, "switch_prob": 1e-3}
PLANTED_RANGE = (-2, 3)


def planted_clones(seed, noise):
    """3 clones x 16 cells over chromosomes of (60, 1, 40, 29) windows: N(0, noise) plus 0.3 x the clone's truth, which
    holds the level steps of PLANTED_SEGMENTS.  dict(x dense float64, chr_pos, truth int8 n x W, clone_truth int8 3 x W,
    codes int64, labels, kwargs)."""
    rng = np.random.default_rng(seed)
    w = sum(PLANTED_LENGTHS)
    clone_truth = np.zeros((3, w), dtype=np.int8)
    for g, a, b, v in PLANTED_SEGMENTS:
        clone_truth[g, a:b] = v
    codes = np.repeat(np.arange(3, dtype=np.int64), PLANTED_CLONE_CELLS)
    truth = clone_truth[codes]
    x = rng.normal(0.0, noise, truth.shape) + PLANTED_STEP * truth
    return {"x": x, "chr_pos": so.chr_pos_of(PLANTED_LENGTHS), "truth": truth, "clone_truth": clone_truth, "codes": codes,
            "labels": np.asarray([f"clone{g}" for g in codes.tolist()], dtype=object), "kwargs": dict(PLANTED_KWARGS)}


def planted_calls(seed, noise):
    """:func:`planted_clones` with ``states``: the per-cell calls of ``_copy_states_oracle.cnv_copy_states``."""
    c = planted_clones(seed, noise)
    c["states"], _, _, c["params"] = co.cnv_copy_states(c["x"], c["chr_pos"], **c["kwargs"])
    return c

"""Numpy / pure-Python oracle of tl.cnv_segments: plain loops over integers.

``S`` is the int8 ``n x W`` matrix of loss (-1) / neutral (0) / gain (+1) calls, ``bounds`` the sorted chromosome starts
followed by ``W``.

1. Runs.  Window t of row i *starts* a run iff ``S[i,t] != 0`` and (t is a chromosome start or ``S[i,t-1] != S[i,t]``);
   it *ends* a run iff ``S[i,t] != 0`` and (``t+1 == W`` or t+1 is a chromosome start or ``S[i,t+1] != S[i,t]``).  The
   k-th start and the k-th end of a row are segment k: ``[start, end+1)`` with state ``S[i,start]``.
2. Order: by row, then by start; ``offsets[i]`` (int64) = the number of segments in the rows < i.
3. ``min_windows`` drops the shorter segments afterwards (a mask on the finished table).
4. Votes: ``loss[g,w]`` / ``gain[g,w]`` (int32) = the cells of group g with S = -1 / +1 at window w; ``n_g`` its cells.
5. Consensus: ``need_g = max(1, ceil(Fraction(min_fraction) n_g))``; +1 if ``gain >= need_g`` and ``gain > loss``; -1 if
   ``loss >= need_g`` and ``loss > gain``; else 0.
6. Group segments: rules 1-2 on the consensus; ``cells_min`` / ``cells_sum`` = the minimum / the int64 sum over the
   segment's windows of the winning state's count; ``support = cells_sum / (n_windows n_g)``, one float64 division.
"""
import math
from fractions import Fraction

import numpy as np


def bounds(chr_pos, n_windows):
    return sorted(int(v) for v in chr_pos.values()) + [int(n_windows)]


def segments(S, edges):
    """Rules 1-2: dict(counts int64 n, offsets int64 n + 1, row int64, start int32, end int32, state int8)."""
    S = np.asarray(S)
    n, w = S.shape
    chrom_start = set(int(e) for e in edges[:-1])
    rows, starts, ends, states, counts = [], [], [], [], []
    for i in range(n):
        r = S[i].tolist()
        st, en = [], []
        for t in range(w):
            if r[t] == 0:
                continue
            if t == 0 or t in chrom_start or r[t - 1] != r[t]:  # (window 0 is a chromosome start)
                st.append(t)
            if t + 1 == w or (t + 1) in chrom_start or r[t + 1] != r[t]:
                en.append(t)
        assert len(st) == len(en)
        for a, b in zip(st, en):
            rows.append(i)
            starts.append(a)
            ends.append(b + 1)
            states.append(r[a])
        counts.append(len(st))
    counts = np.asarray(counts, dtype=np.int64).reshape(n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    return {"counts": counts, "offsets": offsets, "row": np.asarray(rows, dtype=np.int64),
            "start": np.asarray(starts, dtype=np.int32), "end": np.asarray(ends, dtype=np.int32),
            "state": np.asarray(states, dtype=np.int8)}


def need(min_fraction, n_g):
    """rule 5: the votes a state needs in a group of n_g cells."""
    return max(1, math.ceil(Fraction(min_fraction) * int(n_g)))


def votes(S, codes, n_groups):
    """Rule 4: (loss int32 G x W, gain int32 G x W, n_cells int64 G); a code of -1 is no group."""
    S = np.asarray(S)
    n, w = S.shape
    loss = np.zeros((n_groups, w), dtype=np.int32)
    gain = np.zeros((n_groups, w), dtype=np.int32)
    n_cells = np.zeros(n_groups, dtype=np.int64)
    for i in range(n):
        g = int(codes[i])
        if g < 0:
            continue
        n_cells[g] += 1
        loss[g] += S[i] == -1  # one cell's votes, window by window
        gain[g] += S[i] == 1
    return loss, gain, n_cells


def consensus(loss, gain, n_cells, min_fraction):
    """Rule 5: int8 G x W."""
    out = np.zeros(loss.shape, dtype=np.int8)
    for g in range(loss.shape[0]):
        nd = need(min_fraction, n_cells[g])
        for t in range(loss.shape[1]):
            lo, ga = int(loss[g, t]), int(gain[g, t])
            if ga >= nd and ga > lo:
                out[g, t] = 1
            elif lo >= nd and lo > ga:
                out[g, t] = -1
    return out


def group_segments(S, codes, n_groups, edges, min_fraction=0.5):
    """Rules 4-6: the dict of :func:`segments` for the consensus matrix (``row`` is the group) plus loss, gain, n_cells,
    consensus, cells_min int32, cells_sum int64, n_windows int32, support float64."""
    loss, gain, n_cells = votes(S, codes, n_groups)
    cons = consensus(loss, gain, n_cells, min_fraction)
    out = segments(cons, edges) if n_groups else segments(np.zeros((0, np.asarray(S).shape[1]), dtype=np.int8), edges)
    cmin, csum = [], []
    for g, a, b, s in zip(out["row"].tolist(), out["start"].tolist(), out["end"].tolist(), out["state"].tolist()):
        v = (gain if s > 0 else loss)[g, a:b].tolist()
        cmin.append(min(v))
        csum.append(sum(v))
    out.update(loss=loss, gain=gain, n_cells=n_cells, consensus=cons,
               cells_min=np.asarray(cmin, dtype=np.int32), cells_sum=np.asarray(csum, dtype=np.int64))
    out["n_windows"] = (out["end"] - out["start"]).astype(np.int32)
    out["support"] = np.asarray([float(c) / float(int(k) * int(n_cells[g]))
                                 for c, k, g in zip(csum, out["n_windows"].tolist(), out["row"].tolist())],
                                dtype=np.float64)
    return out


def paint(shape, row, start, end, state):
    """The matrix whose segments are the given ones: zeros with ``state`` written over ``[start, end)`` of ``row``."""
    out = np.zeros(shape, dtype=np.int8)
    for i, a, b, s in zip(np.asarray(row).tolist(), np.asarray(start).tolist(), np.asarray(end).tolist(),
                          np.asarray(state).tolist()):
        assert not out[i, a:b].any()
        out[i, a:b] = s
    return out

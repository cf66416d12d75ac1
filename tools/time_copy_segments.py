"""Times of tl.cnv_copy_segments at the geometry of the tl.cnv_copy_states figures (100 000 cells x 1 802 windows in 23
chromosomes, 13 % stored entries; the levels and P(neutral) HBM-resident as tl.cnv_copy_states and tl.cnv_copy_posteriors
leave them).

    python tools/time_copy_segments.py [--groups 6,500] [--cells 100000] [--windows 1802] [--density 0.13] [--reps 20]
                                       [--limit 300]

With several numbers of groups every one runs in a child process of its own under --limit seconds, one after the other; a
child that fails or runs out of time ends the script.  One child prints one JSON line: device-event times (median and
minimum over --reps launches after a warm-up) of icv_level_segments_count, icv_level_segments_fill, icv_level_votes,
icv_level_consensus, icv_level_segments_support and icv_segments_psum; in the same run, as yardsticks, of
icv_segments_count, icv_segments_fill and icv_state_votes on the sign plane of the same calls and of
icv_copy_states_filter on the same levels and posteriors; the ratios between them; and host-clock times of the public
call on device input for both tables.  No time is a pass condition."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def one_form(a, G):
    import pandas as pd
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib
    from infercnvpy_amd._compat import SimpleAnnData
    from time_pca import synthetic_packed
    from time_states import chromosome_bounds

    n, w = a.cells, a.windows
    bounds = chromosome_bounds(w)
    n_chr = int(bounds.shape[0]) - 1
    codes = np.random.default_rng(0).integers(0, G, size=n)
    ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obs=pd.DataFrame({"clone": pd.Categorical(codes)}))
    ad.obsm["X_cnv"] = synthetic_packed(n, w, a.density)
    ad.uns["cnv"] = {"chr_pos": {f"chr{c + 1}": int(s) for c, s in enumerate(bounds[:-1])}}
    cnv.tl.cnv_copy_states(ad)
    cnv.tl.cnv_copy_posteriors(ad)
    del ad.obsm["X_cnv"]
    d_S, d_sign, d_P = (ad.obsm[k] for k in ("X_cnv_copy_states", "X_cnv_copy_states_sign", "X_cnv_copy_posterior_neutral"))
    assert d_S.is_cuda and d_sign.is_cuda and d_P.is_cuda and d_P.dtype == torch.float64
    par = ad.uns["cnv_copy_states"]["params"]
    lo, hi = -int(par["neutral"]), len(par["levels"]) - 1 - int(par["neutral"])
    planes = hi - lo + 1

    lib = _lib.load()
    ptr, st = _engine._ptr, _engine._stream_ptr(torch)
    cs = torch.from_numpy(bounds).cuda()
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    bad = torch.empty(1, dtype=torch.int32, device="cuda")

    def tables(count_entry, fill_entry, S, extra):
        """(count, fill, n_segments, the four tables) of one pair of entries on the matrix S."""
        def count():
            _lib.check(count_entry(ptr(S), n, w, ptr(cs), n_chr, *extra, ptr(counts), ptr(bad), st))

        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        count()
        _lib.check(lib.icv_row_offsets(ptr(counts), n, ptr(offsets), st))
        k = int(offsets[-1].item())
        assert int(bad.item()) == 0
        t = [torch.empty(k, dtype=d, device="cuda") for d in (torch.int64, torch.int32, torch.int32, torch.int8)]

        def fill():
            _lib.check(fill_entry(ptr(S), n, w, ptr(cs), n_chr, ptr(offsets), k, *(ptr(v) for v in t), st))

        return count, fill, k, t

    sign_count, sign_fill, n_sign, _ = tables(lib.icv_segments_count, lib.icv_segments_fill, d_sign, ())
    level_count, level_fill, n_seg, (seg_row, seg_start, seg_end, seg_level) = tables(
        lib.icv_level_segments_count, lib.icv_level_segments_fill, d_S, (lo, hi))

    psum = torch.empty(n_seg, dtype=torch.int64, device="cuda")

    def psum_():
        _lib.check(lib.icv_segments_psum(ptr(d_P), n, w, ptr(seg_row), ptr(seg_start), ptr(seg_end), n_seg, ptr(psum), ptr(bad), st))

    filtered, sign_out = (torch.empty((n, w), dtype=torch.int8, device="cuda") for _ in range(2))
    kept, removed = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))

    def filter_():
        _lib.check(lib.icv_copy_states_filter(ptr(d_S), ptr(d_P), n, w, ptr(cs), n_chr, 0.5, ptr(filtered), ptr(sign_out),
                                              ptr(kept), ptr(removed), ptr(bad), st))

    rows = torch.from_numpy(np.argsort(codes, kind="stable").astype(np.int64)).cuda()
    n_cells = np.bincount(codes, minlength=G)
    group_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64)).cuda()
    need = torch.from_numpy(np.maximum(1, -(-n_cells // 2)).astype(np.int32)).cuda()
    lcounts = torch.empty((G, planes, w), dtype=torch.int32, device="cuda")
    loss, gain = (torch.empty((G, w), dtype=torch.int32, device="cuda") for _ in range(2))
    consensus = torch.empty((G, w), dtype=torch.int8, device="cuda")

    def level_votes():
        _lib.check(lib.icv_level_votes(ptr(d_S), n, w, ptr(rows), n, ptr(group_ptr), G, lo, hi, ptr(lcounts), ptr(bad), st))

    def state_votes():
        _lib.check(lib.icv_state_votes(ptr(d_sign), n, w, ptr(rows), n, ptr(group_ptr), G, ptr(loss), ptr(gain), ptr(bad), st))

    def level_consensus():
        _lib.check(lib.icv_level_consensus(ptr(lcounts), ptr(need), G, w, lo, hi, ptr(loss), ptr(gain), ptr(consensus), st))

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms)}

    def clocked(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": statistics.median(t), "ms_min": min(t)}

    out = {"cells": n, "windows": w, "chromosomes": n_chr, "groups": G, "level_range": [lo, hi], "planes": planes,
           "segments": n_seg, "sign_segments": n_sign, "segments_per_row": n_seg / n, "reps": a.reps,
           "nonneutral_fraction": float((d_S != 0).float().mean().item())}
    out["level_segments_count"] = timed(level_count)
    out["segments_count"] = timed(sign_count)
    out["level_segments_fill"] = timed(level_fill)
    out["segments_fill"] = timed(sign_fill)
    out["segments_psum"] = dict(timed(psum_), bytes_read=int(8 * (seg_end - seg_start).sum().item()) + 16 * n_seg)
    out["copy_states_filter"] = dict(timed(filter_), bytes=11 * n * w)
    assert int(bad.item()) == 0
    out["level_votes"] = timed(level_votes)
    out["state_votes"] = timed(state_votes)
    level_votes(), state_votes()
    # the (group, plane, window) cells that are not 0: each takes one atomic from every row block with rows of the group
    out["votes_nonzero_cells"] = {"level": int((lcounts != 0).sum().item()),
                                  "state": int((loss != 0).sum().item() + (gain != 0).sum().item())}
    out["level_consensus"] = timed(level_consensus)
    level_consensus()
    g_tables = _engine.level_segments_tables(consensus, bounds, lo, hi)
    g_row, g_start, g_end, g_level = g_tables[2:6]
    k = int(g_row.shape[0])
    cmin, lmin = (torch.empty(k, dtype=torch.int32, device="cuda") for _ in range(2))
    csum, lsum = (torch.empty(k, dtype=torch.int64, device="cuda") for _ in range(2))

    def support():
        _lib.check(lib.icv_level_segments_support(ptr(g_row), ptr(g_start), ptr(g_end), ptr(g_level), k, ptr(lcounts),
                                                  ptr(loss), ptr(gain), G, w, lo, hi, ptr(cmin), ptr(csum), ptr(lmin),
                                                  ptr(lsum), st))

    out["group_segments"] = k
    out["level_segments_support"] = timed(support)
    out["call_cells"] = clocked(lambda: cnv.tl.cnv_copy_segments(ad, inplace=False))
    out["call_cells_without_p_neutral"] = clocked(lambda: cnv.tl.cnv_copy_segments(ad, posterior_key=None, inplace=False))
    out["call_groups"] = clocked(lambda: cnv.tl.cnv_copy_segments(ad, "clone", inplace=False))
    for name, num, den in (("level_count_over_count", "level_segments_count", "segments_count"),
                           ("level_fill_over_fill", "level_segments_fill", "segments_fill"),
                           ("psum_over_filter", "segments_psum", "copy_states_filter"),
                           ("level_votes_over_state_votes", "level_votes", "state_votes")):
        out[name] = out[num]["ms_median"] / out[den]["ms_median"]
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="6,500")
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=1802)
    ap.add_argument("--density", type=float, default=0.13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds one number of groups may take")
    a = ap.parse_args()
    forms = [int(v) for v in a.groups.split(",")]
    if len(forms) == 1:
        one_form(a, forms[0])
        return 0
    for G in forms:  # one child per form, one after the other: the first that fails ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--groups", str(G), "--cells", str(a.cells), "--windows",
               str(a.windows), "--density", str(a.density), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"time_copy_segments: {G} groups ran past {a.limit} s", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f"time_copy_segments: {G} groups ended with status {r.returncode}", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Planted inputs for the gene-value kernels (``k_gene_fused``; ``k_gene_means`` -> ``k_row_median`` -> ``k_gene_finish``).

Plans with ``window_size == step`` average ONE window per run (``count == 1``): the run values are then the windows
themselves and a row of the window matrix is a planted multiset.  Values are dyadic rationals (multiples of 2^-20,
|v| <= 8) unless a pattern says otherwise, so ``val - med`` is exact.  ``tests/test_gene_oracle.py`` proves on the CPU,
through the host restatements of the two searches (``_gene_oracle.median_path`` / ``row_median_path``), that every pattern
reaches the branch it is named for; ``tests/test_gpu_gene_values_edges.py`` runs them on both routes.
"""
import numpy as np

import cases

U = 2.0 ** -20
EXTRA = (("chrX", 7), (None, 3))  # columns without a value: NaN in the layer

# name -> (genes per chromosome, window_size, step)
GEOMETRY = {
    # one gene per run, one window per run: R = n_cov = W
    "odd": ([200, 101, 50], 1, 1),         # n_cov 351, n_cols 361
    "even": ([200, 102, 50], 1, 1),        # n_cov 352, n_cols 362
    # runs of 8 genes next to runs of 1..7 genes (chromosomes no longer than the window: one window, all its genes) and
    # chromosome lengths that the step does not divide (their last genes have no value)
    "weighted": ([803, 405, 13, 1, 2, 3, 4, 5, 6, 7], 8, 8),
    # runs of 300 genes: run lengths as 16-bit words in LDS
    "heavy": ([650, 300, 120, 40, 9], 300, 300),   # W = R = 6
    "heavy3": ([650, 120], 300, 300),              # W = 3: odd, the scratch is larger than the windows
    "light4": ([250, 100, 33], 100, 100),          # W = 4, every run <= 255 genes
    # ~5000 runs: the run table stays in memory (pk_lds off), W > 2048 (window loads beyond the prefetch), W odd
    "wide": ([6001, 3000, 1003], 2, 2),
    # k_row_median's bisection needs n_cov > 1024
    "rm_even": ([1000, 400, 100], 1, 1),
    "rm_odd": ([1000, 401, 100], 1, 1),
    # run sums
    "sum128": ([300, 40], 128, 1),          # every count 1..128, the fused kernel
    "sum300": ([700, 420, 25], 300, 1),     # counts pass 128: the round-1 kernels by themselves, n_cov > 1024
}


def annotation(name):
    genes, window, step = GEOMETRY[name]
    v = cases.synthetic_var(genes, extra=EXTRA)
    return v["chromosome"], v["start"], window, step


def make_plan(name):
    from infercnvpy_amd._plan import GenePlan

    chrom, start, window, step = annotation(name)
    return GenePlan(chrom, start, window_size=window, step=step)


# ---------------------------------------------------------------------------------------------------------------------
# planted multisets for n unit-weight runs
# ---------------------------------------------------------------------------------------------------------------------
def spread(m, a, b):
    """m distinct multiples of U, evenly over [a, b]."""
    if m <= 0:
        return np.zeros(0)
    v = np.floor(np.linspace(a, b, m) / U) * U
    assert m == 1 or (np.diff(v) > 0).all()
    return v


def centred(n, core, shift=0):
    """``core`` (values in (-1, 2)) with the rest of the n values around it: outliers -8 and 8 that set the level-0 range,
    the others spread over [-7, -1] and [2, 7]; ``(n - len(core)) // 2 + shift`` values lie below the core."""
    core = np.asarray(core, dtype=np.float64)
    nb = (n - len(core)) // 2 + shift
    na = n - len(core) - nb
    assert nb >= 1 and na >= 1 and core.min() > -1 and core.max() < 2
    return np.concatenate([[-8.0], spread(nb - 1, -7, -1), core, spread(na - 1, 2, 7), [8.0]])


def _nested():
    """99 values in ONE level-0 bin of [-8, 8], 91 of them in one bin of their own range, 71 of those in one bin of the next
    range (multiples of 2^-50 near 1: not of 2^-20): three refinements before the candidates."""
    b0 = 1 + 2.0 ** -10
    c = b0 + 50 * 2.0 ** -30 + np.arange(71) * 2.0 ** -50
    b = np.concatenate([b0 + np.arange(10) * 2.0 ** -30, c, b0 + np.arange(90, 100) * 2.0 ** -30])
    a = np.concatenate([1 + np.arange(4) * 2.0 ** -13, b, 1 + 2.0 ** -9 - np.arange(4)[::-1] * 2.0 ** -13])
    return a


def _ends(end, level=None, first_gt=None, levels_ge=None, last_bin=None, last_count=None, any_k2=False):
    """(any_k2: whether rank k2 lies in the last bin as well is not what the pattern is about)"""
    def check(p):
        assert (p["end"].split("+")[0] if any_k2 else p["end"]) == end, p
        if level is not None:
            assert len(p["counts"]) == level, p
        if first_gt is not None:
            assert p["counts"][0] > first_gt, p
        if levels_ge is not None:
            assert len(p["counts"]) >= levels_ge, p
        if last_bin is not None:
            assert p["bins"][-1] == last_bin, p
        if last_count is not None:
            assert p["counts"][-1] == last_count, p
    return check


def planted(n):
    """name -> (values for n unit-weight runs, check of ``median_path``'s result).  n >= 300; some patterns exist for even
    n only (they need two different middle elements)."""
    assert n >= 300
    even = n % 2 == 0
    k1 = (n - 1) // 2
    x1 = np.nextafter(1.0, np.inf)
    p = {}
    p["all_equal"] = (np.full(n, 1.5), _ends("equal", level=0))
    # two distinct values: bins 0 and 2047 of level 0, both crowded; the tie is found at level 1
    p["two_low"] = (np.r_[np.full(n // 2 + 1, -0.75), np.full(n - n // 2 - 1, 2.25)], _ends("equal", level=1, last_bin=0))
    p["two_high"] = (np.r_[np.full((n - 1) // 2, -0.75), np.full(n - (n - 1) // 2, 2.25)],
                     _ends("equal", level=1, last_bin=2047))
    if even:  # the weight split exactly at the middle: k1 is the last of the low value, k2 the first of the high one
        p["two_split"] = (np.r_[np.full(n // 2, -0.75), np.full(n // 2, 2.25)], _ends("equal+next_above", level=1))
    # 200 values inside one level-0 bin (the range is set by the outliers): one refinement
    p["crowded200"] = (centred(n, 1 + 16 * U * np.arange(200)), _ends("candidates", level=2, first_gt=199, any_k2=True))
    p["cand64"] = (centred(n, 1 + 16 * U * np.arange(64)), _ends("candidates", level=1, last_count=64, any_k2=True))
    p["cand65"] = (centred(n, 1 + 16 * U * np.arange(65)), _ends("candidates", level=2, first_gt=64, any_k2=True))
    p["nested"] = (centred(n, _nested()), _ends("candidates", levels_ge=4, first_gt=64, any_k2=True))
    # > 64 EQUAL values at the median, the rest spread out: refine, then every remaining element equals lo
    p["tie"] = (centred(n, np.full(80, 1.0)), _ends("equal", level=1, first_gt=64))
    if even:
        # the tie's last element is rank k1: k2 is the smallest value above (in another bin / in the tie's own bin)
        nb = k1 - 79
        p["tie_k2_past"] = (centred(n, np.full(80, 1.0), shift=nb - (n - 80) // 2), _ends("equal+next_above", level=1))
        p["tie_k2_past_same_bin"] = (centred(n, np.r_[np.full(80, 1.0), 1.0 + U], shift=nb - (n - 81) // 2),
                                     _ends("equal+next_above", level=2))
        # all values in bins of their own: the two middle elements in different bins
        p["mid_two_bins"] = (spread(n, -4, 4), _ends("candidates+next_above", level=1, last_count=1))
        v = spread(n, -4, 4)
        v[n // 2] = v[k1] + U
        p["mid_one_bin"] = (v, _ends("candidates", level=1, last_count=2))
    else:
        p["mid_alone"] = (spread(n, -4, 4), _ends("candidates", level=1, last_count=1))
    # the median element in bin 0 / in bin 2047 (v == hi: the clamp)
    m = n // 2 + 10
    p["low_majority"] = (np.r_[np.full(m, -3.0), spread(n - m, -2.5, 5)], _ends("equal", level=1, last_bin=0))
    p["high_majority"] = (np.r_[spread(n - m, -3, 4.5), np.full(m, 5.0)], _ends("equal", level=1, last_bin=2047))
    # two adjacent doubles (not multiples of 2^-20)
    p["adjacent_low"] = (np.r_[np.full(n // 2 + 1, 1.0), np.full(n - n // 2 - 1, x1)], _ends("equal", level=1, last_bin=0))
    p["adjacent_high"] = (np.r_[np.full((n - 1) // 2, 1.0), np.full(n - (n - 1) // 2, x1)],
                          _ends("equal", level=1, last_bin=2047))
    if even:
        p["adjacent_split"] = (np.r_[np.full(n // 2, 1.0), np.full(n // 2, x1)], _ends("equal+next_above", level=1))
    return p


def subnormal(n):
    """Zero together with the smallest subnormal: 2048 / (hi - lo) overflows."""
    tiny = 5e-324
    p = {"subnormal_low": (np.r_[np.zeros(n // 2 + 1), np.full(n - n // 2 - 1, tiny)], _ends("equal", level=1, last_bin=0)),
         "subnormal_high": (np.r_[np.zeros((n - 1) // 2), np.full(n - (n - 1) // 2, tiny)],
                            _ends("equal", level=1, last_bin=2047))}
    if n % 2 == 0:
        p["subnormal_split"] = (np.r_[np.zeros(n // 2), np.full(n // 2, tiny)], _ends("equal+next_above", level=1))
    return p


def shuffled(patterns, seed=7):
    """-> (names, rows x n matrix): every pattern's values in a fixed random order (the position of a value among the
    runs is not what the patterns are about; a sorted row would hide an indexing mistake)."""
    rng = np.random.RandomState(seed)
    names = list(patterns)
    return names, np.vstack([patterns[k][0][rng.permutation(len(patterns[k][0]))] for k in names])


def small_rows(n):
    """Every assignment of three values to n <= 6 windows (3^n rows): all ties a handful of weighted runs can have."""
    assert n <= 6
    idx = np.indices((3,) * n).reshape(n, -1).T
    return np.array([-1.5, 0.25, 3.0])[idx]


def dyadic(rows, n, seed):
    """Random multiples of U in [-8, 8]."""
    rng = np.random.RandomState(seed)
    return rng.randint(-8 * 2 ** 20, 8 * 2 ** 20 + 1, size=(rows, n)).astype(np.float64) * U


# ---------------------------------------------------------------------------------------------------------------------
# k_row_median's own limits: n > 1024 unit-weight runs
# ---------------------------------------------------------------------------------------------------------------------
def _rm(end, iters=None, iters_gt=None, key_space=False):
    def check(p):
        assert p["end"] == end, p
        if iters is not None:
            assert p["iters"] == iters, p
        if iters_gt is not None:
            assert p["iters"] > iters_gt, p
        if key_space:
            assert p["key_space"] > 0, p
    return check


def row_median_planted(n):
    """name -> (values, check of ``row_median_path``'s result) for n > 1024 + 400 unit-weight runs."""
    assert n >= 1500
    even = n % 2 == 0
    x1 = np.nextafter(1.0, np.inf)
    p = {}
    p["rm_all_equal"] = (np.full(n, 1.5), _rm("adjacent", iters=0))
    p["rm_tie1100"] = (centred(n, np.full(1100, 1.0)), _rm("adjacent"))
    p["rm_adjacent_low"] = (np.r_[np.full(1100, 1.0), np.full(n - 1100, x1)], _rm("adjacent", iters=1))
    p["rm_adjacent_high"] = (np.r_[np.full(n - 1100, 1.0), np.full(1100, x1)], _rm("adjacent", iters=1))
    # 60 halvings of [-8, 8] do not separate consecutive doubles at 2^-40: the bisection goes on over the keys
    tight = 2.0 ** -40 * (1 + np.arange(n - 2) * 2.0 ** -52)
    assert (np.diff(tight.view(np.int64)) == 1).all()
    p["rm_tight"] = (np.r_[-8.0, tight, 8.0], _rm("candidates", iters_gt=60, key_space=True))
    # consecutive doubles near 1 alone: one pivot leaves <= 1024 candidates (odd n) or falls between the middle two (even n)
    near1 = (np.float64(1.0).view(np.int64) + np.arange(n)).view(np.float64)
    p["rm_consecutive"] = (near1, _rm("separated" if even else "candidates", iters=1))
    if even:
        p["rm_adjacent_split"] = (np.r_[np.full(n // 2, 1.0), np.full(n // 2, x1)], _rm("separated", iters=1))
        # the first pivot (about 0) falls between the two middle elements
        p["rm_pivot_between"] = (np.r_[spread(n // 2, -4, -1), spread(n // 2, 1, 4)], _rm("separated", iters=1))
    return p


# ---------------------------------------------------------------------------------------------------------------------
# run sums: windows whose sum depends on the order of the additions
# ---------------------------------------------------------------------------------------------------------------------
def order_sensitive(rows, n, seed):
    """+-2^e * m with e from -30..30 and a 53-bit m: any other association of a sum changes its bits."""
    rng = np.random.RandomState(seed)
    m = rng.randint(2 ** 52, 2 ** 53, size=(rows, n), dtype=np.int64).astype(np.float64)
    e = rng.randint(-30, 31, size=(rows, n))
    s = np.where(rng.randint(0, 2, size=(rows, n)) == 1, 1.0, -1.0)
    return s * np.ldexp(m, e - 52)


def sequential_run_values(runs, w):
    """The run values of one row with every sum taken left to right: what ``np.add.reduce`` must NOT equal too often."""
    out = np.empty(len(runs["first"]))
    for r, (f, c) in enumerate(zip(runs["first"], runs["count"])):
        acc = 0.0
        for x in w[f:f + c]:
            acc += float(x)
        out[r] = acc / c
    return out


# ---------------------------------------------------------------------------------------------------------------------
# noise filter: run values at med +- thr, one ulp inside and one ulp outside, for EVERY chunk's threshold in every row
# ---------------------------------------------------------------------------------------------------------------------
FILTER_THR = np.array([0.5, 0.25, 1.0])
FILTER_MED = 0.25


def filter_rows(rows, n, seed=11):
    """rows x n run values with median FILTER_MED (symmetric around it): for every t of FILTER_THR the values
    med +- t (|a| == t: kept by the strict <), their neighbours towards the median (zeroed) and away from it (kept);
    the rest are multiples of U.  A row treated with another chunk's threshold gives another row."""
    rng = np.random.RandomState(seed)
    half = n // 2
    out = np.empty((rows, n))
    for i in range(rows):
        up, dn = [], []
        for t in FILTER_THR:
            hi, lo = FILTER_MED + t, FILTER_MED - t
            up += [hi, np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf)]
            dn += [lo, np.nextafter(lo, np.inf), np.nextafter(lo, -np.inf)]
        k = half - len(up)
        stride = 4 * 2 ** 20 // k
        fill = (np.arange(k) * stride + rng.randint(1, stride, size=k)) * U  # distinct, in (0, 4)
        vals = np.r_[np.array(dn), FILTER_MED - fill, np.array(up), FILTER_MED + fill]
        if n % 2:
            vals = np.r_[vals, FILTER_MED]
        out[i] = vals[rng.permutation(n)]
    return out

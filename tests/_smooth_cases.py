"""Inputs on which the smoothing kernels make no rounding error, and their answers from a table (no GPU code).

``k_smooth_x16``, ``k_smooth_ws`` and ``k_smooth_se`` find a cell's median with a histogram, hand a cell back to the
generic ``k_smooth`` when more than 64 windows share the bins of the two middle ranks, and form the noise-threshold
moments per cell or per chunk.  Against gamma-distributed expression they can only be held to 1e-6, and every median
of such data sits in the middle of the central histogram segment.  Two families of inputs make exact tests possible:

Piecewise-constant cells.  ``x = ref + v_c`` on every gene of chromosome c, ``ref`` a multiple of 2^-4 in [0, 4] and
``v_c`` a multiple of 2^-14: the float32 subtraction is exact, every window of chromosome c -- pyramid or flat -- is
exactly ``clip(v_c)`` (the weighted sum ``den * v_c`` is exact and its quotient by ``den`` is correctly rounded), so the
windows, the median, x_res (float32 of the float64 difference) and the cell's sum and sum of squares are a table that
needs neither a kernel nor the oracle.  A chromosome with more genes than the window has ``(G_c - window) // step + 1``
windows, any shorter one has 1: "exactly 64 windows tie at the median" is a choice of chromosome lengths.

Dyadic cells.  ``ref`` and ``x - ref`` multiples of 2^-4 with ``|x - ref| <= 8``: every block sum, window sum and
``np.convolve`` partial is exactly representable in any order and the quotient is correctly rounded, so the float64
oracle (``oracle/infercnv_oracle.py``) is a bit-exact reference for windows, median and x_res of the kernels that keep
the canonical order (x16, ws, generic).

The two bin maps are restated here in numpy float32 ONLY to choose inputs and to assert that a case is what its name
says (which bins the plateaus fall in, how many windows share the median bins); no expected value comes from them.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import cases

CLIP = 3.0
f32, f64 = np.float32, np.float64

# windows per chromosome (chr1 .. chr15): every count a median case needs, and subsets of the rest that put exactly the
# wanted number of windows below the median
WINDOWS = (64, 65, 33, 32, 31, 100, 101, 24, 23, 1, 2, 3, 5, 7, 11)
FLAT_GENES = 57  # the chromosome with one (flat) window


def _genes(window, step, counts):
    return [FLAT_GENES if m == 1 else window + 5 + step * (m - 1) for m in counts]


class Layout:
    """Gene annotation (permuted column order, 3 genes without a chromosome), window counts and the reference row."""

    def __init__(self, name, window, step, fine, n_flat=0):
        self.name, self.window, self.step, self.fine = name, window, step, fine
        # n_flat further chromosomes of exactly `window` genes: one flat window each
        self.counts = list(WINDOWS) + [1] * n_flat
        self.genes = _genes(window, step, WINDOWS) + [window] * n_flat
        for g, m in zip(self.genes, self.counts):
            assert m == ((g - window) // step + 1 if g > window else 1)
        v = cases.synthetic_var(self.genes, seed_start=11, seed_perm=12, extra=((None, 3),))
        self.chromosome, self.start = v["chromosome"], v["start"]
        self.G = len(self.chromosome)
        assert self.G % 4 == 0, "the vector kernels need a multiple of 4 columns"
        self.n_chr = len(self.genes)
        self.cols = [np.flatnonzero(self.chromosome == f"chr{c + 1}") for c in range(self.n_chr)]
        self.free = np.flatnonzero(np.array([c is None for c in self.chromosome]))
        self.W = int(sum(self.counts))
        self.k1, self.k2 = (self.W - 1) // 2, self.W // 2
        rng = np.random.default_rng(5)
        self.ref = (rng.integers(0, 65, self.G) / 16.0).astype(f32)  # multiples of 2^-4 in [0, 4]
        self.first = np.concatenate([[0], np.cumsum(self.counts)[:-1]])  # first window of every chromosome

    def chrom_of_windows(self, m):
        """Index of the chromosome with m windows (the first one)."""
        return self.counts.index(m)


@functools.lru_cache(maxsize=None)
def layout(name):
    if name == "L100":
        L = Layout(name, 100, 10, 4096)
        assert (L.G, L.W, L.k1, L.k2) == (6400, 502, 250, 251)
    elif name == "L100_odd":
        L = Layout(name, 100, 10, 4096, n_flat=1)
        assert (L.G, L.W, L.k1, L.k2) == (6500, 503, 251, 251)
    elif name == "L250":
        # k_smooth_x16 takes its FINE = 1024 histogram only where the 4096-bin one does not fit LDS beside the row
        # (more than about 16 500 genes; with 8 500 genes a window-250 plan runs the generic kernel): 34 flat
        # chromosomes of 250 genes bring the row to 17 000 genes
        L = Layout(name, 250, 10, 1024, n_flat=34)
        assert (L.G, L.W, L.k1, L.k2) == (17000, 536, 267, 268)
    else:
        raise KeyError(name)
    return L


# --------------------------------------------------------------------------------------------------------------- #
# the table
# --------------------------------------------------------------------------------------------------------------- #
Cell = namedtuple("Cell", "x windows median x64 x_res s q")

_Q = 2.0 ** 15  # the median of multiples of 2^-14 is a multiple of 2^-15, and so is every centred window


def is_grid(v, bits=14):
    v = np.asarray(v, dtype=f64)
    return bool(np.all(v * 2.0 ** bits == np.rint(v * 2.0 ** bits)))


def table_cell(L, values):
    """The float32 row ``ref + v_c`` and what every kernel must return for it: windows (float64, before centring),
    median, ``x64 = windows - median``, ``x_res = float32(x64)``, and the exact sum and sum of squares of x64."""
    values = np.asarray(values, dtype=f64)
    assert values.shape == (L.n_chr,) and is_grid(values) and np.abs(values).max() <= 8.0
    x = L.ref.astype(f64)
    for c in range(L.n_chr):
        x[L.cols[c]] += values[c]
    x[L.free] += 1.0  # (genes without a chromosome take no part)
    x32 = x.astype(f32)
    assert np.array_equal(x32.astype(f64), x)
    assert np.array_equal((x32 - L.ref).astype(f64), x - L.ref.astype(f64))  # the kernels' float32 subtraction is exact
    win = np.repeat(np.clip(values, -CLIP, CLIP), L.counts)
    s = np.sort(win)
    med = s[L.k1] if L.k1 == L.k2 else (s[L.k1] + s[L.k2]) / 2.0
    x64 = win - med
    yi = np.rint(x64 * _Q).astype(np.int64)
    assert np.array_equal(yi / _Q, x64)
    qi = int((yi * yi).sum())
    assert qi < 2 ** 53
    return Cell(x32, win, med, x64, x64.astype(f32), float(yi.sum()) / _Q, float(qi) / (_Q * _Q))


def chunk_moments_exact(cells):
    """Exact (sum, sum of squares) over the cells of a chunk as integers over 2^15 / 2^30: every partial sum of a kernel
    is bounded by the totals, so when the totals fit 53 bits any summation order gives the same float64."""
    si = sum(int(round(c.s * _Q)) for c in cells)
    qi = sum(int(round(c.q * _Q * _Q)) for c in cells)
    bound = sum(int(np.abs(np.rint(c.x64 * _Q)).sum()) for c in cells)
    assert qi < 2 ** 53 and bound < 2 ** 53
    return si / _Q, qi / (_Q * _Q)


def chunk_thr(s, q, n_rows, W, dyn):
    """The library's threshold formula (``k_chunk_thr``), restated."""
    n = float(n_rows) * float(W)
    mean = s / n
    var = (q - s * mean) / n
    return dyn * np.sqrt(max(var, 0.0))


def chunk_rows(n, chunksize, row_phase):
    """Rows of every chunk: chunk k holds the rows r with ``(r + row_phase) // chunksize == k``."""
    k = (np.arange(n) + row_phase) // chunksize
    return [np.flatnonzero(k == j) for j in range(int(k.max()) + 1)]


# --------------------------------------------------------------------------------------------------------------- #
# the two bin maps, restated in float32 (to choose inputs and to check what a case is -- never an expected value)
# --------------------------------------------------------------------------------------------------------------- #
def _bound(clip):
    return clip * 1.000001 + 1e-30


def _fma32(a, b, c):
    """float32 fma of float32 arrays: product and sum are exact in float64 for the operands used here (plateau values
    are multiples of 2^-14), so the one rounding is that of the conversion."""
    return (a.astype(f64) * f64(b) + f64(c)).astype(f32)


def hist_bin_x(v, fine, clip=CLIP, frac=False):
    """``hist_bin_x<FINE>`` of ``k_smooth_x16``: the central quarter of [-bound, bound] gets 3/4 of the bins."""
    T = fine // 8
    f = np.atleast_1d(np.asarray(v, dtype=f64)).astype(f32)
    inv_bound = f32(1.0 / _bound(clip))
    c_scale = f32(inv_bound * f32(f32(3 * fine // 4) / f32(0.25)))
    c_thr = f32(f32(0.125) * f32(_bound(clip)))
    central = np.abs(f) < c_thr
    pos_c = _fma32(f, c_scale, fine // 2)
    u = f * f32(f32(0.125) / c_thr)
    k = f32(f32(T) / f32(0.875))
    pos_n = (u + f32(1.0)) * k
    pos_p = _fma32(u - f32(0.125), k, fine - T)
    pos = np.where(central, pos_c, np.where(u < 0, pos_n, pos_p)).astype(f64)
    lo = np.where(central, T, np.where(u < 0, 0, fine - T))
    hi = np.where(central, fine - T - 1, np.where(u < 0, T - 1, fine - 1))
    b = np.clip(np.floor(pos), lo, hi).astype(np.int64)
    return (b, pos - np.floor(pos)) if frac else b


def hist_bin(v, clip=CLIP, frac=False):
    """``hist_bin`` of the 4096-bin kernels (``k_smooth_ws``, ``k_smooth_se``)."""
    f = np.atleast_1d(np.asarray(v, dtype=f64)).astype(f32)
    inv_bound = f32(1.0 / _bound(clip))
    u = f * inv_bound
    central = np.abs(u) < f32(0.125)
    pos_c = _fma32(u, f32(3072.0 / 0.25), 512.0 + 0.125 * (3072.0 / 0.25))
    k = f32(f32(512.0) / f32(0.875))
    pos_n = (u + f32(1.0)) * k
    pos_p = _fma32(u - f32(0.125), k, 3584.0)
    pos = np.where(central, pos_c, np.where(u < 0, pos_n, pos_p)).astype(f64)
    lo = np.where(central, 512, np.where(u < 0, 0, 3584))
    hi = np.where(central, 3583, np.where(u < 0, 511, 4095))
    b = np.clip(np.floor(pos), lo, hi).astype(np.int64)
    return (b, pos - np.floor(pos)) if frac else b


MAPS = {"x1024": lambda v, **kw: hist_bin_x(v, 1024, **kw), "x4096": lambda v, **kw: hist_bin_x(v, 4096, **kw),
        "h4096": lambda v, **kw: hist_bin(v, **kw)}


def map_of(L, route):
    """The bin map a route's kernel uses on layout L (None: the generic kernel has none)."""
    return {"x16": f"x{L.fine}", "ws": "h4096", "se": "h4096", "generic": None}[route]


def is_safe(v, room=0.0):
    """At least 0.1 bin away from a bin edge in every map (float rounding cannot move the plateau; ``room``: further
    bins kept free above it); ``v = 0`` is the exception: ``fmaf(0, c_scale, FINE / 2)`` is exactly ``FINE / 2``, the
    first bin of a coarse bin."""
    if v == 0.0:
        return True
    vc = float(np.clip(v, -CLIP, CLIP))
    if abs(vc) == CLIP:  # clipped: the first / last bin, by the clamps
        return True
    return all(0.1 <= float(m(vc, frac=True)[1][0]) <= 0.9 - room for m in MAPS.values())


def nudge(v, step=2.0 ** -14, room=0.0):
    """The multiple of ``step`` nearest to v that is safe (:func:`is_safe`)."""
    v = round(v / step) * step
    for k in range(256):
        for cand in (v + k * step, v - k * step):
            if is_safe(cand, room):
                return cand
    raise AssertionError(f"no safe plateau value near {v}")


def median_bins(L, windows, which):
    """(b1, b2, nin) of a cell under map ``which``: the bins of the two middle ranks and how many windows lie in them
    (what the kernels compare with 64)."""
    s = np.sort(np.asarray(windows))
    bins = MAPS[which](np.asarray(windows))
    b1, b2 = int(MAPS[which](s[L.k1])[0]), int(MAPS[which](s[L.k2])[0])
    nin = int((bins == b1).sum()) + (int((bins == b2).sum()) if b2 != b1 else 0)
    return b1, b2, nin


def handed_back(L, windows, route):
    """Does the kernel of ``route`` hand this (NaN-free) cell back?"""
    which = map_of(L, route)
    return False if which is None else median_bins(L, windows, which)[2] > 64


# --------------------------------------------------------------------------------------------------------------- #
# median cases
# --------------------------------------------------------------------------------------------------------------- #
def _subset(items, target):
    """Indices into ``items`` (list of (key, count)) whose counts sum to ``target``, or None."""
    reach = {0: []}
    for i, (_, m) in enumerate(items):
        for tot, idx in list(reach.items()):
            if tot + m <= target and tot + m not in reach:
                reach[tot + m] = idx + [i]
    return reach.get(target)


def _fill(L, fixed, n_below, lo, hi):
    """Values for all chromosomes: ``fixed`` {chromosome: value}; of the others a subset with exactly ``n_below`` windows
    gets distinct values below ``lo`` (at least 0.25 away), the rest distinct values above ``hi``."""
    others = [(c, L.counts[c]) for c in range(L.n_chr) if c not in fixed]
    pick = _subset(others, n_below)
    if pick is None:
        return None
    values = np.zeros(L.n_chr)
    for c, v in fixed.items():
        values[c] = v
    below = [others[i][0] for i in pick]
    above = [c for c, _ in others if c not in below]
    for i, c in enumerate(below):
        values[c] = lo - 0.25 - i / 64.0
    for i, c in enumerate(above):
        values[c] = hi + 0.25 + i / 64.0
    return values


MedianCase = namedtuple("MedianCase", "name values kind ma mb place")

# where the two plateaus lie: (name, lower value, upper value)
PLACES = (
    ("same_fine", 2.0 ** -14, 2.0 ** -13),                 # one fine bin: the exact ranking is among distinct values
    ("two_fine", 2.0 ** -10, 2.0 ** -9),                   # two fine bins of one coarse bin
    ("two_coarse", -(2.0 ** -10), 0.0),                    # two coarse bins: the C != Cprev branch of the scan
    ("seam_pos", 0.375, 0.375 + 2.0 ** -10),               # last central bin | first bin of the upper tail
    ("seam_neg", -(0.375 + 2.0 ** -10), -0.375),           # the mirror image
    ("tail_pos", nudge(1.5), nudge(2.0)),                  # two bins of the upper tail
    ("tail_neg", nudge(-2.0, room=0.3), nudge(-2.0, room=0.3) + 2.0 ** -10),   # one bin of the lower tail
    ("last_bin", round(2.99 * 1024) / 1024.0, 5.0),        # the upper plateau is clipped to +3: the last bin
    ("first_bin", -5.0, -round(2.99 * 1024) / 1024.0),     # the mirror image: the first bin
)
PAIRS = ((33, 31), (33, 32), (1, 64), (64, 1), (1, 2), (100, 101))
TIE_VALUE = nudge(73 * 2.0 ** -10)


def tie_case(L, m):
    """One chromosome with m windows ties at the median: both middle ranks fall inside its plateau."""
    t = L.chrom_of_windows(m)
    for off in sorted(range(m), key=lambda o: abs(o - m // 2)):  # windows of the plateau below rank k1, centred first
        n_below = L.k1 - off
        if n_below < 0 or n_below + m <= L.k2:
            continue
        values = _fill(L, {t: TIE_VALUE}, n_below, TIE_VALUE, TIE_VALUE)
        if values is not None:
            return MedianCase(f"tie{m}", values, "tie", m, 0, "tie")
    raise AssertionError(f"{L.name}: no subset puts the middle ranks into the chromosome with {m} windows")


def pair_case(L, place, ma, mb):
    """Two plateaus share the middle ranks: rank k1 is the last window of the lower one (``ma`` windows), k2 the first
    of the upper one (``mb`` windows).  In the first-bin / last-bin places every chromosome beyond the clipped plateau
    is clipped to the same value, so that plateau holds all the windows on its side of the median."""
    assert L.k2 == L.k1 + 1
    name, lo, hi = next(p for p in PLACES if p[0] == place)
    a, b = L.chrom_of_windows(ma), L.chrom_of_windows(mb)
    values = _fill(L, {a: lo, b: hi}, L.k1 + 1 - ma, lo, hi)
    assert values is not None, f"{L.name}: no subset leaves rank k1 on the last of {ma} windows"
    return MedianCase(f"{name}_{ma}_{mb}", values, "pair", ma, mb, name)


@functools.lru_cache(maxsize=None)
def median_cases(layout_name):
    L = layout(layout_name)
    out = [tie_case(L, 64), tie_case(L, 65)]
    if L.k1 != L.k2:
        out += [pair_case(L, p[0], ma, mb) for p in PLACES for ma, mb in PAIRS]
    return out


def check_case(L, case, which):
    """Assert that ``case`` is what its name says under bin map ``which``; returns nin (windows in the median bins)."""
    cell = table_cell(L, case.values)
    s = np.sort(cell.windows)
    b1, b2, nin = median_bins(L, cell.windows, which)
    fine = {"x1024": 1024, "x4096": 4096, "h4096": 4096}[which]
    T = fine // 8
    if case.kind == "tie":
        assert s[L.k1] == s[L.k2] == TIE_VALUE and (cell.windows == TIE_VALUE).sum() == case.ma
        assert b1 == b2 and nin == case.ma
        return nin
    lo, hi = s[L.k1], s[L.k2]
    name, vlo, vhi = next(p for p in PLACES if p[0] == case.place)
    assert lo == np.clip(vlo, -CLIP, CLIP) and hi == np.clip(vhi, -CLIP, CLIP) and lo < hi
    n_lo, n_hi = int((cell.windows == lo).sum()), int((cell.windows == hi).sum())
    assert s[L.k1 + 1 - n_lo] == lo and (L.k1 - n_lo < 0 or s[L.k1 - n_lo] < lo)  # k1 is the LAST window of its plateau
    assert s[L.k2 + n_hi - 1] == hi and (L.k2 + n_hi >= L.W or s[L.k2 + n_hi] > hi)  # k2 the FIRST of its plateau
    if name == "last_bin":
        assert n_lo == case.ma and n_hi == L.W - L.k2 and b2 == fine - 1 and b1 >= fine - 2  # (FINE = 1024: one bin)
    elif name == "first_bin":
        assert n_hi == case.mb and n_lo == L.k1 + 1 and b1 == 0 and b2 <= 1
    else:
        assert (n_lo, n_hi) == (case.ma, case.mb)
        assert nin == case.ma + case.mb, "no other plateau shares the median bins"
    if name == "same_fine":
        assert b1 == b2
    elif name == "two_fine":
        assert b1 != b2 and b1 >> 6 == b2 >> 6
    elif name == "two_coarse":
        assert b1 >> 6 != b2 >> 6 and b2 == fine // 2
    elif name == "seam_pos":
        assert (b1, b2) == (fine - T - 1, fine - T)
    elif name == "seam_neg":
        assert (b1, b2) == (T - 1, T)
    elif name == "tail_pos":
        assert fine - T <= b1 < b2 < fine - 1
    elif name == "tail_neg":
        assert 0 < b1 == b2 < T
    return nin


# --------------------------------------------------------------------------------------------------------------- #
# dyadic (plain) cells and the mixed matrix of the pipeline tests
# --------------------------------------------------------------------------------------------------------------- #
def dyadic_rows(L, n, seed):
    """n float32 rows ``ref + d``, d a multiple of 2^-4 with |d| <= 8 (about a third of the genes clipped at +-3)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-128, 129, (n, L.G)) / 16.0
    d[rng.random((n, L.G)) < 0.5] = 0.0
    x = (L.ref.astype(f64)[None, :] + d).astype(f32)
    assert np.array_equal(x.astype(f64), L.ref.astype(f64)[None, :] + d)
    return x


def oracle_rows(L, X, dynamic_threshold=None, chunk=True):
    """(windows, median, x64, thr) of rows X from the float64 oracle, one chunk.  ``chunk=False``: the windows are
    smoothed once and centred here as ``infercnv_chunk`` centres them (``smoothed - np.median(smoothed, axis=1)``; the
    CPU tests check that the two agree) -- half the time for the large matrices."""
    from oracle import infercnv_oracle as O

    keep = np.array([c is not None for c in L.chromosome])
    ch, st = L.chromosome[keep], L.start[keep]
    centred = np.clip(O.center_on_reference(X[:, keep], L.ref[None, keep]), -CLIP, CLIP)
    _, win = O.smooth_all_chromosomes(centred, ch, st, L.window, L.step)
    med = np.median(win, axis=1)
    if not chunk:
        assert dynamic_threshold is None
        return win, med, win - med[:, np.newaxis], None
    _, res, _, thr = O.infercnv_chunk(X[:, keep], ch, st, L.ref[None, keep], CLIP, L.window, L.step, dynamic_threshold)
    return win, med, res, thr


PLAIN, HANDED, NAN = 0, 1, 2
Mixed = namedtuple("Mixed", "X kind windows median x64 x_res stats")


def _adjacency_ok(kind, cu, grids=(1, 2, 4)):
    n = len(kind)
    for grid in (g * cu for g in grids):
        pairs = {(int(a), int(b)) for a, b in zip(kind[:-grid], kind[grid:])} if n > grid else set()
        if len(pairs) < 9:
            return False
    t = {(int(a), int(b), int(c)) for a, b, c in zip(kind[:-2 * cu], kind[cu:-cu], kind[2 * cu:])}
    if len(t) < 27:
        return False
    # a special cell is the first and the last of some workgroup; so is a plain one
    return len(set(kind[:cu].tolist())) == 3 and len(set(kind[-cu:].tolist())) == 3


@functools.lru_cache(maxsize=4)
def mixed_matrix(layout_name, cu, rows_per_cu=10, seed=0, grids=(1, 2, 4)):
    """About ``rows_per_cu * cu`` rows: a third plain dyadic cells (expected values from the oracle), a third cells that
    every histogram kernel hands back (nonzero piecewise-constant: from the table), a third cells with one NaN gene;
    the types assigned by a seeded shuffle such that, for grids of cu, 2 cu and 4 cu workgroups (``grids``), every
    ordered pair of types occurs among consecutive cells of some workgroup, and at grid cu every ordered triple."""
    L = layout(layout_name)
    n = rows_per_cu * cu
    n -= n % 3
    base = np.repeat(np.array([PLAIN, HANDED, NAN]), n // 3)
    for s in range(seed, seed + 50):
        kind = np.random.default_rng(s).permutation(base)
        if _adjacency_ok(kind, cu, grids):
            break
    else:
        raise AssertionError("no shuffle puts every pair and triple of cell types next to each other")
    rng = np.random.default_rng(1000 + seed)
    hb_cases = [c for c in median_cases(layout_name)
                if all(median_bins(L, table_cell(L, c.values).windows, m)[2] > 64 for m in (f"x{L.fine}", "h4096"))
                and np.abs(table_cell(L, c.values).x64).max() > 0]
    assert len(hb_cases) >= 8
    hb_cells = [table_cell(L, c.values) for c in hb_cases]
    X = dyadic_rows(L, n, 77 + seed)
    W = L.W
    windows, median = np.zeros((n, W)), np.zeros(n)
    x64, stats = np.zeros((n, W)), np.zeros((n, 2))
    covered = []  # genes that lie in some kept window (the last few of a long chromosome lie in none)
    for c in range(L.n_chr):
        order = L.cols[c][np.argsort(L.start[L.cols[c]], kind="stable")]
        covered.append(order[: (L.counts[c] - 1) * L.step + L.window] if L.genes[c] > L.window else order)
    on_chrom = np.concatenate(covered)
    hb_rows = np.flatnonzero(kind == HANDED)
    for i, r in enumerate(hb_rows):
        c = hb_cells[i % len(hb_cells)]
        X[r] = c.x
        windows[r], median[r], x64[r], stats[r] = c.windows, c.median, c.x64, (c.s, c.q)
    for r in np.flatnonzero(kind == NAN):
        X[r, rng.choice(on_chrom)] = np.nan
    rest = np.flatnonzero(kind != HANDED)
    with np.errstate(invalid="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            w, m, res, _ = oracle_rows(L, X[rest], chunk=False)
    windows[rest], median[rest], x64[rest] = w, m, res
    stats[rest, 0], stats[rest, 1] = res.sum(axis=1), (res * res).sum(axis=1)
    nan_rows = np.flatnonzero(kind == NAN)
    assert np.isnan(median[nan_rows]).all() and np.isnan(windows[nan_rows]).any(axis=1).all()
    assert not np.isnan(median[kind != NAN]).any()
    for r in np.flatnonzero(kind == PLAIN)[:64]:  # plain cells stay on the fast path (a handful of candidates)
        for m in (f"x{L.fine}", "h4096"):
            assert median_bins(L, windows[r], m)[2] <= 64
    return Mixed(X, kind, windows, median, x64, x64.astype(f32), stats)


# --------------------------------------------------------------------------------------------------------------- #
# the three-FMA quotient of finish_window, in exact rationals
# --------------------------------------------------------------------------------------------------------------- #
def fma3_quotient(acc, den):
    """``q = RN(acc * rcp); r = RN(acc - q * den); RN(q + r * rcp)`` with ``rcp = RN(1 / den)``: every operation exact
    in rationals, then rounded once (``float(Fraction)`` rounds to nearest even)."""
    from fractions import Fraction as F

    rcp = 1.0 / den
    q = float(F(acc) * F(rcp))
    r = float(F(acc) - F(q) * F(den))
    return float(F(q) + F(r) * F(rcp))

"""numpy oracle of tl.leiden: DESIGN.md 4.10 restated (the specification; leidenalg / igraph are not available).

Every quantity the decisions depend on is an int64 sum (exact, order-free) or ONE float64 expression of such sums
evaluated without fused multiply-add, so a parallel kernel that follows the same schedule gets the same labels.

Graph of a level: n vertices, canonical CSR of the off-diagonal entries (int64 weights > 0), loop[i] = A_ii,
k_i = loop[i] + sum_j w_ij, M = 2m = sum_i k_i (the same at every level), gom = resolution / double(M).

gain(v: a -> c)   = double(k_vc - k_va) - (gom * double(k_v)) * double(K_c - K_a + k_v)        (k_va without the loop)
wellconn(E, K, T) = double(E) >= (gom * double(K)) * double(T - K)
prio(v)           = mix(s + G (v + 1)),  s = mix(mix(mix(seed + G (64 it + level + 1)) + G (phase + 1)) + G (round + 1))
                    (splitmix64's finaliser; phase 0 = local moving, 1 = refinement); v beats u when
                    (prio(v), -v) > (prio(u), -u).

One round of a phase: every vertex decides from the same snapshot.  A wanting vertex v is blocked by a wanting
neighbour u that beats it when their moves touch: u is coming to v's label or u leaves the label v wants (so no swap and
no target that moves away).  In local moving only the wanting vertices whose prio has its top bit set take part in the
round (this breaks the symmetric oscillation of non-adjacent vertices that are coupled through K_c).
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

SCALE_BITS = 32
MAX_LEVELS = 64
MAX_ITERATIONS = 64
G64 = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def max_rounds(n):
    """Bound on the rounds of one phase at a level of n vertices."""
    return 64 + min(int(n), 4096)


def _mix_int(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def round_base(seed, it, level, phase, rnd):
    s = _mix_int((seed & MASK) + G64 * (64 * it + level + 1))
    s = _mix_int(s + G64 * (phase + 1))
    return _mix_int(s + G64 * (rnd + 1))


def prio(s, n):
    with np.errstate(over="ignore"):
        v = np.arange(1, n + 1, dtype=np.uint64)
        return _mix(np.uint64(s) + np.uint64(G64) * v)


# ---- rule 1 / 2: the graph and its integer weights --------------------------------------------------------------------
def quantise(graph, use_weights=True):
    """(indptr int64, indices int32, w int64) of rule 1-2; ValueError for each violation."""
    a = sp.csr_matrix(graph)
    if a.shape[0] != a.shape[1]:
        raise ValueError("tl.leiden: the adjacency matrix must be square")
    a = a.copy()
    a.sum_duplicates()
    a.sort_indices()
    with np.errstate(over="ignore"):
        v = a.data.astype(np.float32)
    if not np.isfinite(v).all():
        raise ValueError("tl.leiden: the adjacency matrix has non-finite values")
    if (v < 0).any():
        raise ValueError("tl.leiden: the adjacency matrix has negative values")
    n = a.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(a.indptr))
    if (rows == a.indices).any():
        raise ValueError("tl.leiden: the adjacency matrix has stored diagonal entries")
    b = sp.csr_matrix((v, a.indices, a.indptr), shape=a.shape)
    bt = b.T.tocsr()
    bt.sort_indices()
    if not (np.array_equal(b.indptr, bt.indptr) and np.array_equal(b.indices, bt.indices)
            and np.array_equal(b.data, bt.data)):
        raise ValueError("tl.leiden: the adjacency matrix is not symmetric")
    if not use_weights:
        v = np.ones_like(v)
    if (v >= 2.0 ** 30).any():
        raise ValueError("tl.leiden: the weights are too large (sum of the integer weights must stay below 2^62)")
    w = np.rint(v.astype(np.float64) * 2.0 ** SCALE_BITS).astype(np.int64)
    if sum(int(x) for x in w) >= 1 << 62:
        raise ValueError("tl.leiden: the weights are too large (sum of the integer weights must stay below 2^62)")
    keep = w > 0
    cnt = np.zeros(n, dtype=np.int64)
    np.add.at(cnt, rows[keep], 1)
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return indptr, a.indices[keep].astype(np.int32), w[keep]


class _Level:
    def __init__(self, indptr, indices, w, loop):
        self.n = len(indptr) - 1
        self.indptr, self.col, self.w, self.loop = indptr, indices.astype(np.int64), w, loop
        self.row = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(indptr))
        self.k = loop.copy()
        np.add.at(self.k, self.row, w)


def _segment_sums(key, w):
    """Unique keys (ascending) and the int64 sums of w per key."""
    if len(key) == 0:
        return key, w
    o = np.argsort(key, kind="stable")
    ks, ws = key[o], w[o]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    return ks[start], np.add.reduceat(ws, start)


def _inexact(*ints):
    """How many of the int64 values are not float64 numbers (their conversion rounds)."""
    return sum(int((np.asarray(x).astype(np.float64).astype(np.int64) != x).sum()) for x in ints)


def _gain(gom, dk, kv, dK, stats=None):
    if stats is not None:
        stats["inexact_gain"] += _inexact(dk, kv, dK)
    return dk.astype(np.float64) - (gom * kv.astype(np.float64)) * dK.astype(np.float64)


def _wellconn(gom, E, K, T, stats=None):
    if stats is not None:
        stats["inexact_wellconn"] += _inexact(E, K, T - K)
    return E.astype(np.float64) >= (gom * K.astype(np.float64)) * (T - K).astype(np.float64)


def new_stats():
    """The branch counters `iteration` fills (they only observe):
    empty_rounds          local-moving rounds in which a selected vertex chose EMPTY
    empty_short_rounds    ... in which the selected EMPTY vertices outnumbered the free ids
    empty_got_none        selected EMPTY vertices that got no id (rule 4d, "none if they ran out")
    tie_lower_id          decisions taken whose best gain was shared by another candidate (the lower id won)
    zero_gain_refine      refinement decisions taken at gain == 0 exactly
    refine_candidates_rejected / refine_movers_rejected    by wellconn
    blocked               wanting vertices that took part in a round and lost to a neighbour (rule 4c)
    thinned               wanting vertices left out of a local-moving round by the top priority bit
    row_lengths           per level entered: (level, sorted distinct row lengths)
    inexact_gain / inexact_wellconn   int64 values converted to float64 that were not float64 numbers"""
    s = dict.fromkeys(("empty_rounds", "empty_short_rounds", "empty_got_none", "tie_lower_id", "zero_gain_refine",
                       "refine_candidates_rejected", "refine_movers_rejected", "blocked", "thinned", "inexact_gain",
                       "inexact_wellconn"), 0)
    s["row_lengths"] = []
    return s


EMPTY = -2


def _decide(L, gom, label, KL, cntL, refine, comm=None, Kc=None, ext=None, stats=None):
    """want[v] (target label, EMPTY, or -1) and wantw[v] = k_{v -> target} from the snapshot."""
    n = L.n
    want = np.full(n, -1, dtype=np.int64)
    wantw = np.zeros(n, dtype=np.int64)
    a = label
    ce = label[L.col]
    valid = np.ones(len(ce), dtype=bool) if not refine else comm[L.col] == comm[L.row]
    key, s = _segment_sums(L.row[valid] * n + ce[valid], L.w[valid])
    pv, pc = key // n, key % n
    kva = np.zeros(n, dtype=np.int64)
    own = pc == a[pv]
    kva[pv[own]] = s[own]
    if refine:
        single = cntL[a] == 1
        mover = single & _wellconn(gom, ext, L.k, Kc[comm], stats)
        cand = _wellconn(gom, ext[pc], KL[pc], Kc[comm[pv]], stats)
        ok = ~own & mover[pv] & cand
        if stats is not None:
            stats["refine_movers_rejected"] += int((single & ~mover).sum())
            stats["refine_candidates_rejected"] += int((~own & mover[pv] & ~cand).sum())
    else:
        ok = ~own
    pv, pc, s = pv[ok], pc[ok], s[ok]
    g = _gain(gom, s - kva[pv], L.k[pv], KL[pc] - KL[a[pv]] + L.k[pv], stats)
    o = np.lexsort((pc, -g, pv))
    pv, pc, s, g = pv[o], pc[o], s[o], g[o]
    first = np.flatnonzero(np.concatenate([[True], pv[1:] != pv[:-1]])) if len(pv) else np.zeros(0, dtype=np.int64)
    bv, bc, bs, bg = pv[first], pc[first], s[first], g[first]
    if stats is not None and len(pv):
        nxt = np.minimum(first + 1, len(pv) - 1)
        tied = (nxt > first) & (pv[nxt] == bv) & (g[nxt] == bg)  # the runner-up has the same gain: the lower id won
    best_g = np.full(n, -np.inf)
    best_g[bv] = bg
    if refine:
        sel = bg >= 0
        want[bv[sel]] = bc[sel]
        wantw[bv[sel]] = bs[sel]
        if stats is not None and len(pv):
            stats["tie_lower_id"] += int((tied & sel).sum())
            stats["zero_gain_refine"] += int((bg == 0).sum())
        return want, wantw
    sel = bg > 0
    want[bv[sel]] = bc[sel]
    has_entries = np.diff(L.indptr) > 0
    ge = _gain(gom, -kva, L.k, L.k - KL[a], stats)
    to_empty = has_entries & (cntL[a] > 1) & (ge > 0) & (ge > best_g)
    want[to_empty] = EMPTY
    if stats is not None and len(pv):
        stats["tie_lower_id"] += int((tied & sel & ~to_empty[bv]).sum())
    return want, wantw


def _select(L, want, label, s, thin, stats=None):
    """Rule 4c: the wanting vertices that move this round."""
    p = prio(s, L.n)
    wants = want != -1
    if thin:
        top = (p >> np.uint64(63)) == 1
        if stats is not None:
            stats["thinned"] += int((wants & ~top).sum())
        wants &= top
    r, c = L.row, L.col
    both = wants[r] & wants[c] & ((want[c] == label[r]) | (label[c] == want[r]))
    r, c = r[both], c[both]
    beats = (p[r] > p[c]) | ((p[r] == p[c]) & (r < c))
    lose = np.zeros(L.n, dtype=bool)
    lose[r[~beats]] = True
    if stats is not None:
        stats["blocked"] += int((wants & lose).sum())
    return np.where(wants & ~lose, want, -1)


def _local_moving(L, gom, comm, seed, it, level, stats=None):
    n = L.n
    K = np.zeros(n, dtype=np.int64)
    np.add.at(K, comm, L.k)
    cnt = np.bincount(comm, minlength=n).astype(np.int64)
    moves, rounds, bound = 0, 0, False
    while True:
        if rounds == max_rounds(n):
            bound = True
            break
        want, _ = _decide(L, gom, comm, K, cnt, False, stats=stats)
        if not (want != -1).any():
            break
        sel = _select(L, want, comm, round_base(seed, it, level, 0, rounds), True, stats)
        rounds += 1
        we = np.flatnonzero(sel == EMPTY)
        if len(we):
            free = np.flatnonzero(cnt == 0)
            m = min(len(we), len(free))
            if stats is not None:
                stats["empty_rounds"] += 1
                stats["empty_short_rounds"] += len(we) > len(free)
                stats["empty_got_none"] += len(we) - m
            sel[we[:m]] = free[:m]
            sel[we[m:]] = -1
        mv = np.flatnonzero(sel >= 0)
        b = sel[mv]
        np.add.at(K, comm[mv], -L.k[mv])
        np.add.at(K, b, L.k[mv])
        np.add.at(cnt, comm[mv], -1)
        np.add.at(cnt, b, 1)
        comm[mv] = b
        moves += len(mv)
    return moves, rounds, bound


def _refine(L, gom, comm, seed, it, level, stats=None):
    n = L.n
    Kc = np.zeros(n, dtype=np.int64)
    np.add.at(Kc, comm, L.k)
    sub = np.arange(n, dtype=np.int64)
    Ks = L.k.copy()
    cs = np.ones(n, dtype=np.int64)
    ext = np.zeros(n, dtype=np.int64)
    same = comm[L.row] == comm[L.col]
    np.add.at(ext, L.row[same], L.w[same])
    rounds, bound = 0, False
    while True:
        if rounds == max_rounds(n):
            bound = True
            break
        want, wantw = _decide(L, gom, sub, Ks, cs, True, comm, Kc, ext, stats)
        if not (want != -1).any():
            break
        sel = _select(L, want, sub, round_base(seed, it, level, 1, rounds), False, stats)
        rounds += 1
        mv = np.flatnonzero(sel >= 0)
        t = sel[mv]
        np.add.at(Ks, t, L.k[mv])
        np.add.at(cs, t, 1)
        np.add.at(ext, t, ext[mv] - 2 * wantw[mv])
        pair = (sel[L.row] >= 0) & (sel[L.row] == sel[L.col])  # two adjacent vertices that join the same target
        np.add.at(ext, sel[L.row[pair]], -L.w[pair])
        Ks[mv], cs[mv], ext[mv] = 0, 0, 0
        sub[mv] = t
    return sub, rounds, bound


def _aggregate(L, comm, sub):
    n = L.n
    vmap = np.cumsum(np.bincount(sub, minlength=n) > 0) - 1
    cmap = np.cumsum(np.bincount(comm, minlength=n) > 0) - 1
    n2 = int(vmap[-1]) + 1
    r = vmap[sub]
    comm2 = np.zeros(n2, dtype=np.int64)
    comm2[r] = cmap[comm]
    loop2 = np.zeros(n2, dtype=np.int64)
    np.add.at(loop2, r, L.loop)
    rr, rc = r[L.row], r[L.col]
    inner = rr == rc
    np.add.at(loop2, rr[inner], L.w[inner])
    key, s = _segment_sums(rr[~inner] * n2 + rc[~inner], L.w[~inner])
    indptr = np.concatenate([[0], np.cumsum(np.bincount(key // n2, minlength=n2))]).astype(np.int64)
    return _Level(indptr, key % n2, s, loop2), comm2, r


def community_sums(indptr, indices, w, labels):
    """(e_c, K_c) int64 per label of the level-0 graph."""
    n = len(indptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    C = int(labels.max()) + 1 if n else 0
    e = np.zeros(C, dtype=np.int64)
    K = np.zeros(C, dtype=np.int64)
    same = labels[row] == labels[indices]
    np.add.at(e, labels[row[same]], w[same])
    np.add.at(K, labels[row], w)
    return e, K


def quality(e, K, resolution):
    """Q of rule 3 from the integer sums (math.fsum: independent of the order)."""
    M = sum(int(x) for x in K)
    if M == 0:
        return 0.0
    Mf = float(M)
    return math.fsum((float(ec) - resolution * float(kc) * float(kc) / Mf) / Mf for ec, kc in zip(e.tolist(), K.tolist()))


def renumber(labels):
    """Rule 6: by decreasing size, ties by the smallest member."""
    n = len(labels)
    if n == 0:
        return labels.astype(np.int32)
    size = np.bincount(labels, minlength=int(labels.max()) + 1)
    first = np.full(len(size), n, dtype=np.int64)
    np.minimum.at(first, labels, np.arange(n))
    order = np.lexsort((first, -size))
    order = order[size[order] > 0]
    new = np.zeros(len(size), dtype=np.int64)
    new[order] = np.arange(len(order))
    return new[labels].astype(np.int32)


def iteration(indptr, indices, w, gom, seed, it, labels, stats=None):
    """ONE iteration (rule 4) of the integer graph from ANY partition `labels` (ids in [0, n)), as icv_leiden_iteration
    runs it: (labels_out int64, not renumbered; vertices per level; (local moving, refinement) rounds per level; the
    local moves of all levels; whether a rule-5 bound was reached).  `stats` (new_stats()) receives the branch counters."""
    n = len(indptr) - 1
    seed = int(seed) & MASK
    L = _Level(np.asarray(indptr, dtype=np.int64), np.asarray(indices), np.asarray(w, dtype=np.int64),
               np.zeros(n, dtype=np.int64))
    comm, o2c = np.array(labels, dtype=np.int64), np.arange(n, dtype=np.int64)
    total, sizes, rnds, bound, done = 0, [], [], False, False
    for level in range(MAX_LEVELS):
        if stats is not None:
            stats["row_lengths"].append((level, np.unique(np.diff(L.indptr))))
        moves, r_move, b1 = _local_moving(L, gom, comm, seed, it, level, stats)
        sub, r_ref, b2 = _refine(L, gom, comm, seed, it, level, stats)
        total += moves
        sizes.append(L.n)
        rnds.append((r_move, r_ref))
        bound |= b1 or b2
        if len(np.unique(sub)) == L.n:
            done = True
            break
        L, comm, r = _aggregate(L, comm, sub)
        o2c = r[o2c]
    return comm[o2c], sizes, rnds, total, bound or not done


def leiden(graph, resolution=1.0, random_state=0, n_iterations=-1, use_weights=True, return_info=False, stats=None):
    """Labels (int32, rule 6) of DESIGN 4.10; with return_info also the dict tl.leiden reports."""
    indptr, indices, w = quantise(graph, use_weights)
    n = len(indptr) - 1
    resolution = float(resolution)
    seed = int(random_state) & MASK
    M = sum(int(x) for x in w)
    info = {"quality": [], "n_iterations": 0, "levels": [], "rounds": [], "bound_reached": False}
    labels = np.arange(n, dtype=np.int64)
    if M > 0:
        gom = resolution / float(M)
        it = 0
        while True:
            if n_iterations > 0 and it == n_iterations:
                break
            if it == MAX_ITERATIONS:
                info["bound_reached"] = info["bound_reached"] or n_iterations < 0
                break
            labels, sizes, rnds, total, bound = iteration(indptr, indices, w, gom, seed, it, labels, stats)
            it += 1
            info["bound_reached"] = info["bound_reached"] or bound
            info["levels"].append(sizes)
            info["rounds"].append(rnds)
            info["quality"].append(quality(*community_sums(indptr, indices, w, renumber(labels)), resolution))
            if n_iterations < 0 and total == 0:
                break
        info["n_iterations"] = it
    out = renumber(labels)
    return (out, info) if return_info else out


# ---- independent checks (scipy products on the int64 weights) ---------------------------------------------------------
def check_partition(labels):
    labels = np.asarray(labels)
    n = len(labels)
    if n == 0:
        return
    C = int(labels.max()) + 1
    size = np.bincount(labels, minlength=C)
    assert labels.min() == 0 and (size > 0).all()
    first = np.full(C, n, dtype=np.int64)
    np.minimum.at(first, labels, np.arange(n))
    for c in range(1, C):
        assert (size[c - 1], -first[c - 1]) > (size[c], -first[c]), c


def check_connected(graph_int, labels):
    """Every community induces a connected subgraph."""
    from scipy.sparse.csgraph import connected_components

    a = graph_int.tocoo()
    keep = labels[a.row] == labels[a.col]
    b = sp.csr_matrix((np.ones(keep.sum(), dtype=np.int8), (a.row[keep], a.col[keep])), shape=a.shape)
    ncomp, _ = connected_components(b, directed=False)
    assert ncomp == int(labels.max()) + 1, (ncomp, int(labels.max()) + 1)


def check_node_optimal(graph_int, labels, resolution):
    """No vertex has a move to a neighbouring or an empty community with gain > 0 (the contract's expression)."""
    labels = np.asarray(labels, dtype=np.int64)
    n = graph_int.shape[0]
    C = int(labels.max()) + 1
    a = graph_int.tocsr().astype(np.int64)
    k = np.asarray(a.sum(axis=1)).ravel().astype(np.int64)
    M = int(sum(int(x) for x in k))
    if M == 0:
        return
    gom = float(resolution) / float(M)
    ind = sp.csr_matrix((np.ones(n, dtype=np.int64), (np.arange(n), labels)), shape=(n, C))
    kvc = (a @ ind).tocoo()  # k_{v -> c} of every neighbouring community
    K = np.asarray(ind.T @ k).ravel()
    size = np.bincount(labels, minlength=C)
    kva = np.zeros(n, dtype=np.int64)
    own = kvc.col == labels[kvc.row]
    kva[kvc.row[own]] = kvc.data[own]
    v, c, s = kvc.row[~own], kvc.col[~own], kvc.data[~own]
    g = _gain(gom, s - kva[v], k[v], K[c] - K[labels[v]] + k[v])
    assert not (g > 0).any(), f"{int((g > 0).sum())} vertices can still move to a neighbouring community"
    ge = _gain(gom, -kva, k, k - K[labels])
    bad = (ge > 0) & (size[labels] > 1)
    assert not bad.any(), f"{int(bad.sum())} vertices can still move to an empty community"


def modularity(graph, labels, resolution):
    """networkx.community.modularity of an undirected weighted graph, on the float64 values (for hosts without
    networkx; test_leiden_oracle.py compares the two where it imports)."""
    g = sp.csr_matrix(graph).astype(np.float64)
    labels = np.asarray(labels)
    k = np.asarray(g.sum(axis=1)).ravel()
    ind = sp.csr_matrix((np.ones(len(labels)), (np.arange(len(labels)), labels)))
    return float(((ind.T @ g @ ind).diagonal() / k.sum() - resolution * (ind.T @ k / k.sum()) ** 2).sum())


def int_graph(graph, use_weights=True):
    indptr, indices, w = quantise(graph, use_weights)
    n = len(indptr) - 1
    return sp.csr_matrix((w, indices, indptr), shape=(n, n))


# ---- test graphs ------------------------------------------------------------------------------------------------------
def _sym(rows, cols, vals, n):
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals, dtype=np.float64)
    a = sp.coo_matrix((np.concatenate([vals, vals]), (np.concatenate([rows, cols]), np.concatenate([cols, rows]))),
                      shape=(n, n)).tocsr()
    a.sort_indices()
    return a


def cliques(sizes, ring=False):
    """Disjoint cliques; ring=True joins clique i to clique i + 1 by one edge."""
    r, c, start = [], [], 0
    starts = []
    for s in sizes:
        i, j = np.triu_indices(s, 1)
        r.append(i + start)
        c.append(j + start)
        starts.append(start)
        start += s
    if ring:
        m = len(sizes)
        r.append(np.array([starts[i] + sizes[i] - 1 for i in range(m)]))
        c.append(np.array([starts[(i + 1) % m] for i in range(m)]))
    r, c = np.concatenate(r), np.concatenate(c)
    return _sym(r, c, np.ones(len(r)), start)


def star(n_leaves):
    return _sym(np.zeros(n_leaves, dtype=np.int64), np.arange(1, n_leaves + 1), np.ones(n_leaves), n_leaves + 1)


def complete(n):
    return cliques([n])


def path(n):
    return _sym(np.arange(n - 1), np.arange(1, n), np.ones(n - 1), n)


def isolated(n):
    return sp.csr_matrix((n, n), dtype=np.float64)


def wide_weights(n=400, seed=0):
    """Random graph whose weights span 2^-30 .. 1: some quantise to small integers, the smallest are dropped."""
    rng = np.random.default_rng(seed)
    m = 6 * n
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = r < c
    r, c = r[keep], c[keep]
    _, first = np.unique(r * n + c, return_index=True)
    r, c = r[first], c[first]
    vals = 2.0 ** (-rng.integers(0, 31, len(r)).astype(np.float64))
    vals[::7] = 2.0 ** -34  # rounds to w = 0: dropped
    return _sym(r, c, vals, n)


def mixture_graph(n, seed=0):
    """pp.neighbors' connectivities (oracle) of _neighbors_oracle.mixture(n, 10, seed), n_neighbors = 15."""
    import _neighbors_oracle as no

    return no.neighbors(no.mixture(n, 10, seed), 15)["connectivities"]


def with_hub(graph, weight=0.01):
    """`graph` plus one vertex joined to every other one (a long row in a graph that has structure)."""
    n = graph.shape[0]
    g = sp.coo_matrix(graph)
    hub = np.full(n, n)
    return _sym(np.concatenate([g.row[g.row < g.col], np.arange(n)]), np.concatenate([g.col[g.row < g.col], hub]),
                np.concatenate([g.data[g.row < g.col].astype(np.float64), np.full(n, weight)]), n + 1)


def small_graphs():
    """name -> graph: every test graph of the issue except the mixtures."""
    return {
        "cliques": cliques([7, 5, 5, 9, 3, 2, 1]),
        "ring_of_cliques": cliques([5] * 30, ring=True),
        "star": star(40),
        "hub5000": star(4999),
        "k300": complete(300),
        "path": path(101),
        "isolated": isolated(17),
        "n1": isolated(1),
        "n2": path(2),
        "wide_weights": wide_weights(),
    }


# ---- edge builders (tests/test_gpu_leiden_edges.py; test_leiden_oracle.py asserts that the oracle reaches each branch) -
def rows_at_split():
    """Rows of 511, 512, 513 and 514 entries: around the 512 at which a row leaves the LDS kernel for the long-row one."""
    return cliques([513, 514, 512], ring=True)


SPLIT_HUBS = (511, 512, 513, 514, 515)


def pairs_with_hubs(pairs=515, hubs=SPLIT_HUBS, weight=2.0 ** -20):
    """`pairs` disjoint edges plus one hub per entry t of `hubs`, joined to the first vertex of the first t edges by a
    light edge.  Every edge becomes one vertex of the aggregate, so the hubs have rows on both sides of 512 entries at
    level 0 AND at level 1."""
    n = 2 * pairs + len(hubs)
    r = [np.arange(0, 2 * pairs, 2)]
    c = [np.arange(1, 2 * pairs, 2)]
    v = [np.ones(pairs)]
    for h, t in enumerate(hubs):
        r.append(np.arange(0, 2 * t, 2))
        c.append(np.full(t, 2 * pairs + h))
        v.append(np.full(t, weight))
    return _sym(np.concatenate(r), np.concatenate(c), np.concatenate(v), n)


def heavy_mixed(n=300, seed=0):
    """Random graph, half of its weights 2^18 (1 + j 2^-23) and half j 2^-32, j in [1, 4096): float32 numbers whose
    integer weights 2^50 + j 2^27 and j add up to sums of more than 53 bits, so the int64 -> float64 conversions of the
    gain and of wellconn round."""
    rng = np.random.default_rng(seed)
    m = 4 * n
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = r < c
    r, c = r[keep], c[keep]
    _, first = np.unique(r * n + c, return_index=True)
    r, c = r[first], c[first]
    j = rng.integers(1, 4096, len(r)).astype(np.float64)
    heavy = rng.permutation(len(r)) < len(r) // 2
    return _sym(r, c, np.where(heavy, 2.0 ** 18 * (1 + j * 2.0 ** -23), j * 2.0 ** -32), n)


def near_limit():
    """name -> graph at the limit sum w < 2^62 of rule 2; the names that start with "over" must raise."""
    r = np.array([0, 1, 2, 3, 4, 0, 1, 2, 0])
    c = np.array([1, 2, 3, 4, 5, 2, 3, 5, 5])
    v = np.array([2.0 ** 27, 2.0 ** 26, 2.0 ** 26 * (1 + 2.0 ** -23), 2.0 ** 27 - 8, 2.0 ** 25, 5 * 2.0 ** -32, 2.0 ** -7,
                  3 * 2.0 ** -32, 2.0 ** 25 * (1 + 2.0 ** -22)])
    return {
        "pair_below": path(2) * (2.0 ** 29 - 32),       # sum w = 2^62 - 2^38
        "mixed_below": _sym(r, c, v, 6),                # sum w = 0.875 2^62, with weights of 3 and 5 in it
        "over_pair": path(2) * 2.0 ** 29,               # sum w = 2^62 exactly, every value below 2^30
        "over_k3": complete(3) * 2.0 ** 29,
    }


def rint_ties():
    """Path whose edge i has the value (i + 1) 2^-33, i < 9: w = rint((i + 1) / 2) with the ties 0.5, 1.5, 2.5, 3.5 and
    4.5 (to even: 0, 2, 2, 4, 4); then a float32 subnormal (w = 0: dropped) and a weight of 1 that closes the ring."""
    vals = np.concatenate([np.arange(1, 10) * 2.0 ** -33, [2.0 ** -140, 1.0]])
    n = len(vals)
    return _sym(np.arange(n), (np.arange(n) + 1) % n, vals, n)


def cycle(n):
    return _sym(np.arange(n), (np.arange(n) + 1) % n, np.ones(n), n)


EMPTIES_GAMMA = 8.0
# (n, members, random_state): found by empties_search(); every `it` of EMPTIES_ITS runs out of free ids with that seed
EMPTIES_ITS = (0, 1, 63)
EMPTIES_CASES = {"two": (12, 2, 13), "five": (14, 5, 8)}


def empties_run_out(n, members):
    """(graph, labels): a cycle of n vertices; `members` non-adjacent vertices (0, 2, 4, ...) share the label 0, every
    other vertex is alone, so members - 1 ids are free.  At gamma = EMPTIES_GAMMA > n / 2 no vertex gains by joining a
    neighbour and every member prefers an empty community: when all of them are selected in one round, one gets none."""
    labels = np.arange(n, dtype=np.int32)
    labels[0:2 * members:2] = 0
    return cycle(n), labels


def empties_search(n, members, seeds=range(4096)):
    """The first random_state of `seeds` at which the case runs out of free ids for every `it` of EMPTIES_ITS."""
    g, labels = empties_run_out(n, members)
    indptr, indices, w = quantise(g)
    gom = EMPTIES_GAMMA / float(sum(int(x) for x in w))
    for seed in seeds:
        for it in EMPTIES_ITS:
            st = new_stats()
            iteration(indptr, indices, w, gom, seed, it, labels, st)
            if st["empty_got_none"] == 0:
                break
        else:
            return seed
    return None


def zero_gain_cases():
    """name -> (graph, gamma): complete graphs in ONE community at gamma = n / (n - 1), where joining a neighbour in the
    refinement has the gain 0 exactly (w - (gamma / (n (n - 1) w)) ((n - 1) w)^2, every product a float64 number): the
    refinement merges at gain >= 0, so the iteration has a second level."""
    return {"k2": (complete(2), 2.0), "k3": (complete(3), 1.5), "k5": (complete(5), 1.25)}


def kv_not_float32():
    """(graph, gamma): the path 0 - 1 - 2 with w_01 = 2^32 and w_12 = 1, so k_1 = 2^32 + 1 is a float64 but no float32
    number, at gamma = 2 (1 + 2^-34): the gain of 1 joining 0 is 2^32 - gom (2^32 + 1) 2^32 = -0.25, no move, and +0.75
    with k_1 rounded to float32.  Nothing moves: the labels are the singletons."""
    return _sym([0, 1], [1, 2], [1.0, 2.0 ** -32], 3), 2.0 * (1 + 2.0 ** -34)


def start_partitions(graph, seed=0):
    """name -> int32 labels (ids in [0, n)) to start `iteration` from; "converged" is added by the tests."""
    n = graph.shape[0]
    rng = np.random.default_rng(seed)
    ids = rng.choice(n, max(n // 9, 2), replace=False)  # ids used sparsely over [0, n)
    return {
        "one": np.zeros(n, dtype=np.int32),
        "gaps": ids[rng.integers(0, len(ids), n)].astype(np.int32),
        "disconnected": (np.arange(n) % 6 * (n // 6)).astype(np.int32),  # every 6th vertex: spread over the graph
    }


def converged(graph, resolution, seed):
    """Labels (not renumbered) after the iterations of leiden(graph, resolution, seed, -1), and how many ran."""
    indptr, indices, w = quantise(graph)
    gom = float(resolution) / float(sum(int(x) for x in w))
    labels = np.arange(len(indptr) - 1, dtype=np.int64)
    for it in range(MAX_ITERATIONS):
        labels, _, _, moves, _ = iteration(indptr, indices, w, gom, seed, it, labels)
        if moves == 0:
            return labels.astype(np.int32), it + 1
    raise AssertionError("not converged")


# ---- rule 5: a seeded search for an input that reaches the round bound -------------------------------------------------
def rule5_shapes():
    """Graphs of up to 12 vertices, among them the symmetric shapes of rule 4c (non-adjacent vertices coupled through
    K_c): complete bipartite graphs, stars, cycles, two hubs that share their leaves."""
    def bipartite(a, b):
        r, c = np.meshgrid(np.arange(a), a + np.arange(b), indexing="ij")
        return _sym(r.ravel(), c.ravel(), np.ones(a * b), a + b)

    out = {f"k{a}_{b}": bipartite(a, b) for a, b in ((2, 2), (2, 5), (2, 10), (3, 3), (3, 9), (4, 4), (4, 8), (6, 6))}
    out.update({f"star{n}": star(n) for n in (3, 7, 11)})
    out.update({f"cycle{n}": cycle(n) for n in (4, 6, 8, 12)})
    out.update({"complete6": complete(6), "complete12": complete(12), "path12": path(12),
                "cliques3x4": cliques([3] * 4, ring=True), "cliques4x3": cliques([4] * 3, ring=True)})
    return out


def rule5_search(budget, seed=0):
    """`budget` cases (shape, optional random weights, starting partition, gamma in [0, 8], random_state, it) drawn from
    default_rng(seed): (the cases that reached a bound, the most rounds of a phase minus that level's bound)."""
    rng = np.random.default_rng(seed)
    shapes = list(rule5_shapes().items())
    gammas = (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0)
    found, closest = [], -10 ** 9
    for case in range(budget):
        name, g = shapes[rng.integers(len(shapes))]
        n = g.shape[0]
        if rng.integers(3) == 0:  # symmetric random weights 2^-k
            u = sp.triu(g).tocoo()
            g = _sym(u.row, u.col, 2.0 ** -rng.integers(0, 12, u.nnz).astype(np.float64), n)
        kind = rng.integers(5)
        labels = (np.arange(n), np.zeros(n, dtype=np.int64), np.arange(n) % 2, np.arange(n) // 2 * 2,
                  rng.integers(0, n, n))[kind]
        gamma, rs, it = gammas[rng.integers(len(gammas))], int(rng.integers(1 << 62)), int(rng.integers(64))
        indptr, indices, w = quantise(g)
        gom = gamma / float(sum(int(x) for x in w))
        _, sizes, rnds, _, bound = iteration(indptr, indices, w, gom, rs, it, labels)
        closest = max(closest, max(max(r) - max_rounds(s) for s, r in zip(sizes, rnds)))
        if bound:
            found.append((case, name, kind, gamma, rs, it))
    return found, closest

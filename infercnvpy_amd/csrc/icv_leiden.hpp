// tl.leiden: Leiden on the device.  Every sum a decision depends on is an int64 (integer atomics, any
// order); the gain and the well-connectedness test are ONE float64 expression each (the library is built
// -ffp-contract=off), so the labels are a pure function of the arguments and equal tests/_leiden_oracle.py bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_graph.hpp"  // ld_mix, ld_wave_sum, kGraphLongRow, graph_entry_flags

namespace icv {

constexpr int kLdEmpty = -2;            // want[v]: an empty community (its id is assigned by rank, rule 4d)
constexpr int kLdMaxLevels = 64;        // levels per iteration (rule 5)
constexpr int kLdLdsRow = kGraphLongRow;  // longest row k_ld_decide combines in LDS; longer rows: k_ld_decide_long

__host__ __device__ __forceinline__ uint64_t ld_prio(uint64_t s, int v) {
    return ld_mix(s + 0x9E3779B97F4A7C15ull * (uint64_t)(v + 1));
}
inline uint64_t ld_round_base(uint64_t seed, int it, int level, int phase, int rnd) {
    const uint64_t g = 0x9E3779B97F4A7C15ull;
    uint64_t s = ld_mix(seed + g * (uint64_t)(64 * it + level + 1));
    s = ld_mix(s + g * (uint64_t)(phase + 1));
    return ld_mix(s + g * (uint64_t)(rnd + 1));
}
__device__ __forceinline__ double ld_gain(double gom, long long dk, long long kv, long long dK) {
    return (double)dk - (gom * (double)kv) * (double)dK;
}
__device__ __forceinline__ bool ld_wellconn(double gom, long long E, long long K, long long T) {
    return (double)E >= (gom * (double)K) * (double)(T - K);
}
__device__ __forceinline__ void ld_add(long long* p, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// ---- rule 1 / 2: validation and the integer weights (a wavefront per row) ---------------------------------------------
// flags: those of graph_entry_flags, and 64 value >= 2^30.  sums[0] / sums[1]: the low / high 32-bit halves of the
// weights, summed.  The lane's accumulated f gates q, as before the per-entry test was shared; the one difference,
// checked against the host's order of reports, is that -inf now sets flag 1 alone (it used to set 1 and 2, and 1 is
// reported first).  A graph that passes has f = 0 in both forms, so wq, row_keep and sums are the same; the outputs
// of one that fails are discarded.
template <typename T>
__global__ __launch_bounds__(256) void k_ld_quantise(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                     const T* __restrict__ val, int64_t n, int use_weights,
                                                     long long* __restrict__ wq, long long* __restrict__ row_keep,
                                                     unsigned* __restrict__ flags, unsigned long long* __restrict__ sums) {
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const int64_t b = indptr[v], e = indptr[v + 1];
    unsigned f = 0;
    long long keep = 0, lo = 0, hi = 0;
    for (int64_t i = b + lane; i < e; i += 64) {
        const float x = (float)val[i];
        f |= graph_entry_flags(indptr, col, val, n, v, b, i, x);
        long long q = 0;
        if (f == 0) {
            const float y = use_weights ? x : 1.f;
            if (y >= 1073741824.f) f |= 64;
            else q = __double2ll_rn((double)y * 4294967296.0);
        }
        wq[i] = q;
        keep += q > 0;
        lo += q & 0xFFFFFFFFll;
        hi += q >> 32;
    }
    for (int off = 32; off > 0; off >>= 1) f |= __shfl_xor(f, off, 64);
    keep = ld_wave_sum(keep);
    lo = ld_wave_sum(lo);
    hi = ld_wave_sum(hi);
    if (lane == 0) {
        row_keep[v] = keep;
        if (f) atomicOr(flags, f);
        if (lo) atomicAdd(&sums[0], (unsigned long long)lo);
        if (hi) atomicAdd(&sums[1], (unsigned long long)hi);
    }
}

// the entries with w > 0, in order
__global__ __launch_bounds__(256) void k_ld_compact(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                    const long long* __restrict__ wq, int64_t n,
                                                    const int64_t* __restrict__ out_ptr, int32_t* __restrict__ out_col,
                                                    long long* __restrict__ out_w) {
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const int64_t b = indptr[v], e = indptr[v + 1];
    int64_t base = out_ptr[v];
    for (int64_t i0 = b; i0 < e; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool k = i < e && wq[i] > 0;
        const unsigned long long m = __ballot(k);
        if (k) {
            const int64_t o = base + __popcll(m & ((1ull << lane) - 1ull));
            out_col[o] = col[i];
            out_w[o] = wq[i];
        }
        base += __popcll(m);
    }
}

// ---- a level ----------------------------------------------------------------------------------------------------------
// k_i (a wavefront per vertex) and the list of the rows that k_ld_decide_long takes (any order: rows are independent)
__global__ __launch_bounds__(256) void k_ld_strength(const int64_t* __restrict__ rowptr, const long long* __restrict__ w,
                                                     const long long* __restrict__ loop, int n, long long* __restrict__ k,
                                                     int32_t* __restrict__ long_list, unsigned* __restrict__ n_long) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const int64_t b = rowptr[v], e = rowptr[v + 1];
    long long s = 0;
    for (int64_t i = b + lane; i < e; i += 64) s += w[i];
    s = ld_wave_sum(s);
    if (lane == 0) {
        k[v] = s + (loop ? loop[v] : 0);
        if (e - b > kLdLdsRow) long_list[atomicAdd(n_long, 1u)] = v;
    }
}

__global__ void k_ld_init_comm(const int32_t* __restrict__ comm, const long long* __restrict__ k, int n,
                               long long* __restrict__ K, int32_t* __restrict__ cnt) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    ld_add(&K[comm[v]], k[v]);
    atomicAdd(&cnt[comm[v]], 1);
}

// (gain, lower id) of two candidates; id 0x7fffffff = none
__device__ __forceinline__ void ld_better(double& bg, int& bc, long long& bs, double g, int c, long long s) {
    if (g > bg || (g == bg && c < bc)) {
        bg = g;
        bc = c;
        bs = s;
    }
}
__device__ __forceinline__ void ld_wave_best(double& bg, int& bc, long long& bs) {
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_xor(bg, off, 64);
        const int oc = __shfl_xor(bc, off, 64);
        const long long os = __shfl_xor(bs, off, 64);
        ld_better(bg, bc, bs, og, oc, os);
    }
}
// what the vertex wants, from its best candidate (rule 3)
template <bool REFINE>
__device__ __forceinline__ void ld_verdict(double gom, double bg, int bc, long long bs, long long kva, long long kv,
                                           long long Ka, int members, int& res, long long& resw) {
    if (REFINE) {
        if (bc != 0x7fffffff && bg >= 0.0) {
            res = bc;
            resw = bs;
        }
    } else {
        if (bc != 0x7fffffff && bg > 0.0) res = bc;
        if (members > 1) {
            const double ge = ld_gain(gom, -kva, kv, kv - Ka);
            if (ge > 0.0 && ge > bg) res = kLdEmpty;
        }
    }
}

// Rule 3 / 4a-b: the best move of every vertex from the snapshot.  A wavefront per vertex; the row's (label, w) pairs
// are staged in LDS once (one gather per entry), the lane that owns the FIRST entry of a label sums that label's weight
// from LDS, the wavefront reduces (gain, id) by shuffles.  Rows above kLdLdsRow entries: k_ld_decide_long.
// counters[0] += wanting.
template <bool REFINE>
__global__ __launch_bounds__(256) void k_ld_decide(int n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                   const long long* __restrict__ w, const long long* __restrict__ k,
                                                   const int32_t* __restrict__ label, const long long* __restrict__ KL,
                                                   const int32_t* __restrict__ cntL, const int32_t* __restrict__ comm,
                                                   const long long* __restrict__ Kc, const long long* __restrict__ ext,
                                                   double gom, int32_t* __restrict__ want, long long* __restrict__ wantw,
                                                   unsigned* __restrict__ counters) {
    __shared__ int s_c[4][kLdLdsRow];
    __shared__ long long s_w[4][kLdLdsRow];
    const int wave = threadIdx.x >> 6;
    const int v = blockIdx.x * 4 + wave;
    const int lane = threadIdx.x & 63;
    int64_t b = 0;
    int deg = 0, a = 0, cv = 0;
    long long kv = 0, T = 0;
    bool in_range = v < n, mover = false;
    if (in_range) {
        b = rowptr[v];
        const int64_t d = rowptr[v + 1] - b;
        if (d > kLdLdsRow) in_range = false;  // k_ld_decide_long writes this vertex
        deg = (int)d;
    }
    if (in_range && deg > 0) {
        a = label[v];
        kv = k[v];
        cv = REFINE ? comm[v] : 0;
        T = REFINE ? Kc[cv] : 0;
        mover = !REFINE || (cntL[a] == 1 && ld_wellconn(gom, ext[v], kv, T));
        if (mover)
            for (int i = lane; i < deg; i += 64) {
                const int u = col[b + i];
                s_c[wave][i] = (REFINE && comm[u] != cv) ? -1 : label[u];
                s_w[wave][i] = w[b + i];
            }
    }
    __syncthreads();
    if (!in_range) return;
    int res = -1;
    long long resw = 0;
    if (mover) {
        long long kva = 0;
        for (int i = lane; i < deg; i += 64)
            if (s_c[wave][i] == a) kva += s_w[wave][i];
        kva = ld_wave_sum(kva);
        double bg = -INFINITY;
        int bc = 0x7fffffff;
        long long bs = 0;
        for (int i = lane; i < deg; i += 64) {
            const int c = s_c[wave][i];
            if (c < 0 || c == a) continue;
            bool first = true;
            for (int j = 0; j < i; ++j)
                if (s_c[wave][j] == c) {
                    first = false;
                    break;
                }
            if (!first) continue;
            if (REFINE && !ld_wellconn(gom, ext[c], KL[c], T)) continue;
            long long s = 0;
            for (int j = i; j < deg; ++j)
                if (s_c[wave][j] == c) s += s_w[wave][j];
            ld_better(bg, bc, bs, ld_gain(gom, s - kva, kv, KL[c] - KL[a] + kv), c, s);
        }
        ld_wave_best(bg, bc, bs);
        ld_verdict<REFINE>(gom, bg, bc, bs, kva, kv, KL[a], cntL[a], res, resw);
    }
    if (lane == 0) {
        want[v] = res;
        wantw[v] = resw;
        if (res != -1) atomicAdd(&counters[0], 1u);
    }
}

// The same decision for a row of ANY length: a workgroup per row of long_list, the row's labels combined in an
// open-addressing table in global memory (the row's own 2 x deg slots of hk / hv: integer atomics, so the sums do
// not depend on the order), then one candidate per occupied slot.
template <bool REFINE>
__global__ __launch_bounds__(256) void k_ld_decide_long(const int32_t* __restrict__ long_list, const int64_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, const long long* __restrict__ w,
                                                        const long long* __restrict__ k, const int32_t* __restrict__ label,
                                                        const long long* __restrict__ KL, const int32_t* __restrict__ cntL,
                                                        const int32_t* __restrict__ comm, const long long* __restrict__ Kc,
                                                        const long long* __restrict__ ext, double gom, int32_t* __restrict__ hk,
                                                        long long* __restrict__ hv, int32_t* __restrict__ want,
                                                        long long* __restrict__ wantw, unsigned* __restrict__ counters) {
    __shared__ double r_g[4];
    __shared__ int r_c[4];
    __shared__ long long r_s[4];
    const int v = long_list[blockIdx.x];
    const int tid = threadIdx.x;
    const int64_t b = rowptr[v], e = rowptr[v + 1];
    const unsigned long long S = 2ull * (unsigned long long)(e - b);
    const int a = label[v];
    const long long kv = k[v];
    const int cv = REFINE ? comm[v] : 0;
    const long long T = REFINE ? Kc[cv] : 0;
    if (REFINE && !(cntL[a] == 1 && ld_wellconn(gom, ext[v], kv, T))) {  // the same for the whole workgroup
        if (tid == 0) {
            want[v] = -1;
            wantw[v] = 0;
        }
        return;
    }
    int32_t* keys = hk + 2 * b;
    long long* vals = hv + 2 * b;
    for (unsigned long long s = tid; s < S; s += 256) {
        keys[s] = -1;
        vals[s] = 0;
    }
    __threadfence();
    __syncthreads();
    for (int64_t i = b + tid; i < e; i += 256) {
        const int u = col[i];
        if (REFINE && comm[u] != cv) continue;
        const int c = label[u];
        unsigned long long s = ((unsigned long long)((unsigned)c * 2654435761u)) % S;
        for (;;) {
            const int prev = atomicCAS(&keys[s], -1, c);
            if (prev == -1 || prev == c) break;
            s = s + 1 == S ? 0 : s + 1;
        }
        ld_add(&vals[s], w[i]);
    }
    __threadfence();
    __syncthreads();
    long long kva = 0;
    {
        unsigned long long s = ((unsigned long long)((unsigned)a * 2654435761u)) % S;
        for (;;) {
            const int key = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (key == a) kva = __hip_atomic_load(&vals[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (key == a || key == -1) break;
            s = s + 1 == S ? 0 : s + 1;
        }
    }
    double bg = -INFINITY;
    int bc = 0x7fffffff;
    long long bs = 0;
    for (unsigned long long s = tid; s < S; s += 256) {
        const int c = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c < 0 || c == a) continue;
        if (REFINE && !ld_wellconn(gom, ext[c], KL[c], T)) continue;
        const long long sum = __hip_atomic_load(&vals[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ld_better(bg, bc, bs, ld_gain(gom, sum - kva, kv, KL[c] - KL[a] + kv), c, sum);
    }
    ld_wave_best(bg, bc, bs);
    if ((tid & 63) == 0) {
        r_g[tid >> 6] = bg;
        r_c[tid >> 6] = bc;
        r_s[tid >> 6] = bs;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; ++i) ld_better(bg, bc, bs, r_g[i], r_c[i], r_s[i]);
        int res = -1;
        long long resw = 0;
        ld_verdict<REFINE>(gom, bg, bc, bs, kva, kv, KL[a], cntL[a], res, resw);
        want[v] = res;
        wantw[v] = resw;
        if (res != -1) atomicAdd(&counters[0], 1u);
    }
}

// Rule 4c: which wanting vertices move (a wavefront per vertex).  counters[1] += selected, counters[2] += selected
// that want an empty community.
__global__ __launch_bounds__(256) void k_ld_select(int n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                   const int32_t* __restrict__ label, const int32_t* __restrict__ want,
                                                   uint64_t s, int thin, int32_t* __restrict__ sel,
                                                   unsigned* __restrict__ counters) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const int wv = want[v];
    const uint64_t p = ld_prio(s, v);
    bool active = wv != -1 && (!thin || (p >> 63));
    if (active) {
        const int lv = label[v];
        const int64_t b = rowptr[v], e = rowptr[v + 1];
        for (int64_t i0 = b; i0 < e; i0 += 64) {
            const int64_t i = i0 + lane;
            bool lose = false;
            if (i < e) {
                const int u = col[i];
                const int wu = want[u];
                if (wu != -1 && (wu == lv || label[u] == wv)) {
                    const uint64_t pu = ld_prio(s, u);
                    lose = (!thin || (pu >> 63)) && (pu > p || (pu == p && u < v));
                }
            }
            if (__any(lose)) {
                active = false;
                break;
            }
        }
    }
    if (lane == 0) {
        sel[v] = active ? wv : -1;
        if (active) {
            atomicAdd(&counters[1], 1u);
            if (wv == kLdEmpty) atomicAdd(&counters[2], 1u);
        }
    }
}

// Rule 4d: the r-th selected vertex (by index) that wants an empty community gets the r-th free id (by id).
__global__ void k_ld_empty_flags(int n, const int32_t* __restrict__ cnt, const int32_t* __restrict__ sel,
                                 int32_t* __restrict__ fa, int32_t* __restrict__ fb) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > n) return;
    fa[v] = v < n && cnt[v] == 0;
    fb[v] = v < n && sel[v] == kLdEmpty;
}
__global__ void k_ld_free_list(int n, const int32_t* __restrict__ cnt, const int32_t* __restrict__ ra,
                               int32_t* __restrict__ free_list) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n && cnt[c] == 0) free_list[ra[c]] = c;
}
__global__ void k_ld_assign_empty(int n, const int32_t* __restrict__ ra, const int32_t* __restrict__ rb,
                                  const int32_t* __restrict__ free_list, int32_t* __restrict__ sel) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n && sel[v] == kLdEmpty) sel[v] = rb[v] < ra[n] ? free_list[rb[v]] : -1;
}

__global__ void k_ld_apply_move(int n, const int32_t* __restrict__ sel, const long long* __restrict__ k,
                                int32_t* __restrict__ comm, long long* __restrict__ K, int32_t* __restrict__ cnt,
                                unsigned long long* __restrict__ moves) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int t = sel[v];
    if (t < 0) return;
    const int a = comm[v];
    ld_add(&K[a], -k[v]);
    ld_add(&K[t], k[v]);
    atomicSub(&cnt[a], 1);
    atomicAdd(&cnt[t], 1);
    comm[v] = t;
    atomicAdd(moves, 1ull);
}

// refinement: singletons, ext[v] = the weight from v to the rest of its community (a wavefront per vertex)
__global__ __launch_bounds__(256) void k_ld_refine_init(int n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const long long* __restrict__ w, const long long* __restrict__ k,
                                                        const int32_t* __restrict__ comm, int32_t* __restrict__ sub,
                                                        long long* __restrict__ Ks, int32_t* __restrict__ cs,
                                                        long long* __restrict__ ext) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    long long s = 0;
    const int c = comm[v];
    for (int64_t i = rowptr[v] + lane; i < rowptr[v + 1]; i += 64)
        if (comm[col[i]] == c) s += w[i];
    s = ld_wave_sum(s);
    if (lane == 0) {
        sub[v] = v;
        Ks[v] = k[v];
        cs[v] = 1;
        ext[v] = s;
    }
}

// a target never moves in the same round (k_ld_select), so its sums only receive; the mover's own slots are cleared
__global__ __launch_bounds__(256) void k_ld_apply_refine(int n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const long long* __restrict__ w, const int32_t* __restrict__ sel,
                                                         const long long* __restrict__ wantw, const long long* __restrict__ k,
                                                         int32_t* __restrict__ sub, long long* __restrict__ Ks,
                                                         int32_t* __restrict__ cs, long long* __restrict__ ext) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const int t = sel[v];
    if (t < 0) return;
    long long d = 0;
    for (int64_t i = rowptr[v] + lane; i < rowptr[v + 1]; i += 64)
        if (sel[col[i]] == t) d -= w[i];  // an adjacent vertex that joins the same target
    d = ld_wave_sum(d);
    if (lane == 0) {
        ld_add(&Ks[t], k[v]);
        atomicAdd(&cs[t], 1);
        ld_add(&ext[t], d + ext[v] - 2 * wantw[v]);
        Ks[v] = 0;
        cs[v] = 0;
        ext[v] = 0;
        sub[v] = t;
    }
}

// ---- aggregation ------------------------------------------------------------------------------------------------------
__global__ void k_ld_used_flags(int n, const int32_t* __restrict__ cs, const int32_t* __restrict__ cnt,
                                int32_t* __restrict__ fa, int32_t* __restrict__ fb) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > n) return;
    fa[v] = v < n && cs[v] > 0;
    fb[v] = v < n && cnt[v] > 0;
}
__global__ void k_ld_agg_vertices(int n, const int32_t* __restrict__ sub, const int32_t* __restrict__ comm,
                                  const int32_t* __restrict__ vmap, const int32_t* __restrict__ cmap,
                                  const long long* __restrict__ loop, int32_t* __restrict__ comm2,
                                  long long* __restrict__ loop2) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int r = vmap[sub[v]];
    comm2[r] = cmap[comm[v]];
    if (loop && loop[v]) ld_add(&loop2[r], loop[v]);
}
// key (new row << 32 | new column) of every entry; an entry inside a vertex of the aggregate goes to its loop
__global__ __launch_bounds__(256) void k_ld_agg_keys(int n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                     const long long* __restrict__ w, const int32_t* __restrict__ sub,
                                                     const int32_t* __restrict__ vmap, unsigned long long* __restrict__ keys,
                                                     long long* __restrict__ vals, long long* __restrict__ loop2) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const unsigned long long r = (unsigned)vmap[sub[v]];
    long long inner = 0;
    for (int64_t i = rowptr[v] + lane; i < rowptr[v + 1]; i += 64) {
        const unsigned long long c = (unsigned)vmap[sub[col[i]]];
        keys[i] = c == r ? ~0ull : (r << 32 | c);
        vals[i] = w[i];
        if (c == r) inner += w[i];
    }
    inner = ld_wave_sum(inner);
    if (lane == 0 && inner) ld_add(&loop2[r], inner);
}
__global__ void k_ld_agg_rowptr(int n2, int64_t nnz2, const unsigned long long* __restrict__ ukeys,
                                int64_t* __restrict__ rowptr2) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n2) return;
    const unsigned long long key = (unsigned long long)r << 32;
    int64_t lo = 0, hi = nnz2;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (ukeys[m] < key) lo = m + 1;
        else hi = m;
    }
    rowptr2[r] = lo;
}
__global__ void k_ld_agg_cols(int64_t nnz2, const unsigned long long* __restrict__ ukeys, int32_t* __restrict__ col2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nnz2) col2[i] = (int32_t)(ukeys[i] & 0xFFFFFFFFull);
}
__global__ void k_ld_o2c(int64_t n0, const int32_t* __restrict__ sub, const int32_t* __restrict__ vmap,
                         int32_t* __restrict__ o2c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n0) o2c[i] = vmap[sub[o2c[i]]];
}
__global__ void k_ld_iota(int64_t n, int32_t* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = (int32_t)i;
}
__global__ void k_ld_gather(int64_t n, const int32_t* __restrict__ table, const int32_t* __restrict__ idx,
                            int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = table[idx[i]];
}

// ---- rule 6 and the quality's integer sums ----------------------------------------------------------------------------
__global__ void k_ld_sizes(int64_t n, const int32_t* __restrict__ labels, int32_t* __restrict__ size,
                           int32_t* __restrict__ first) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atomicAdd(&size[labels[i]], 1);
    atomicMin(&first[labels[i]], (int32_t)i);
}
__global__ void k_ld_size_keys(int64_t n, const int32_t* __restrict__ size, const int32_t* __restrict__ first,
                               unsigned long long* __restrict__ keys, int32_t* __restrict__ ids, unsigned* __restrict__ n_comm) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    ids[c] = (int32_t)c;
    keys[c] = size[c] > 0 ? ((unsigned long long)(n - size[c]) << 32 | (unsigned)first[c]) : ~0ull;
    if (size[c] > 0) atomicAdd(n_comm, 1u);
}
__global__ void k_ld_scatter_rank(int64_t n, const int32_t* __restrict__ ids, int32_t* __restrict__ rank) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rank[ids[i]] = (int32_t)i;
}
__global__ __launch_bounds__(256) void k_ld_sums(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const long long* __restrict__ w, const int32_t* __restrict__ labels,
                                                 long long* __restrict__ e, long long* __restrict__ K) {
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const int c = labels[v];
    long long se = 0, sk = 0;
    for (int64_t i = rowptr[v] + lane; i < rowptr[v + 1]; i += 64) {
        sk += w[i];
        if (labels[col[i]] == c) se += w[i];
    }
    se = ld_wave_sum(se);
    sk = ld_wave_sum(sk);
    if (lane == 0) {
        if (se) ld_add(&e[c], se);
        if (sk) ld_add(&K[c], sk);
    }
}

}  // namespace icv

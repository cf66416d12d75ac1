// tl.cnv_pool_neighbors: every cell's profile averaged with those of its graph neighbours, exactly.  The
// contract (tests/_pool_oracle.py restates it):
//   1. values are those of 4.17 rule 1: stored values are used as float64 (a float32 is promoted exactly), an entry that is
//      not stored is 0, a stored 0.0 or -0.0 adds nothing.
//   2. the neighbourhood of cell i is N(i) = {i} u {indices[e] : indptr[i] <= e < indptr[i + 1]}; an explicit diagonal entry
//      does not count i twice; L_i = |N(i)|; an empty graph row gives N(i) = {i}.  Only the structure of the graph is read.
//   3. shift e in [0, 40] (the caller's min(40, 52 - bit_length(max L_i))); every stored magnitude is < 2^10.
//   4. S[i,w] = the int64 sum over j in N(i) of rint(x[j,w] 2^e), ties to even.  Integer adds: the order does not matter.
//   5. pooled[i,w] = (double(S[i,w]) / double(L_i)) 2^-e: one round-to-nearest-even conversion, one correctly rounded
//      division, an exact scaling.  S = 0 gives +0.0.
//
// Geometry: the windows are cut into tiles of kPoolTile.  One workgroup per (cell, tile) keeps the tile's int64 sums in LDS
// (8 bytes per window, 16 KB: no counts), its sixteen groups of kPoolRowLanes lanes take the rows of N(i) in turn -- position
// 0 is the cell itself, position p > 0 the graph entry p - 1, read straight from the graph row, so a row of any length is
// walked without staging, and the cell with 14 neighbours has all its rows in flight at once -- a group's lanes stride the
// matrix row's stored entries (CSR) or its part of the tile (dense: 16-byte loads from the first 16-byte boundary on, the
// values in front of it and behind the last whole load one by one, as k_group_profiles does) and add into LDS with 64-bit
// LDS atomics.  After one barrier the workgroup converts, divides and writes its tile of the output
// row once: a float64 in front of the first 16-byte boundary of the row's tile (an odd number of windows misaligns every
// second row), 16-byte stores of two windows from there on, one float64 behind them.  No global atomic, no memset, no
// table between the matrix and the result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_pseudobulk.hpp"  // pb_pow2, kPbMaxShift

namespace icv {

constexpr int kPoolTile = 2048;    // windows per workgroup: 8 bytes of LDS each
constexpr int kPoolThreads = 256;  // 4 wavefronts
constexpr int kPoolRowLanes = 16;  // lanes that share one row of the neighbourhood: 16 rows in flight per workgroup
constexpr int kPoolFlagNonfinite = 1, kPoolFlagColumn = 2, kPoolFlagOrder = 4;

// rule 2 per cell, one wavefront per graph row: L_i = 1 + the entries of the row that name another cell of the graph.  A
// column outside [0, n) and a row whose columns do not ascend strictly are flagged (L_i counts a repeated column twice
// then: the caller refuses the graph).
__global__ __launch_bounds__(kPoolThreads) void k_pool_sizes(const int64_t* __restrict__ g_indptr,
                                                             const int32_t* __restrict__ g_indices, int64_t n,
                                                             int32_t* __restrict__ n_cells, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kPoolThreads / 64) + (threadIdx.x >> 6);
    if (i >= n) return;  // (the whole wavefront)
    const int64_t e0 = g_indptr[i], e1 = g_indptr[i + 1];
    int count = 0, f = 0;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int64_t j = g_indices[e];
        if (j < 0 || j >= n) f |= kPoolFlagColumn;
        else if (j != i) ++count;
        if (e > e0 && (int64_t)g_indices[e - 1] >= j) f |= kPoolFlagOrder;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        count += __shfl_xor(count, d, 64);
        f |= __shfl_xor(f, d, 64);
    }
    if (lane == 0) {
        n_cells[i] = count + 1;
        if (f) atomicOr(flags, f);
    }
}

// rules 1 and 4 for one value of window column c of the tile (pb_add without the count)
__device__ __forceinline__ void pool_add(double v, int c, double scale, unsigned long long* s_sum, bool& nonfinite) {
    if (v == 0.0) return;  // (0.0 and -0.0; NaN goes on)
    if (!(__builtin_fabs(v) < __builtin_inf())) {
        nonfinite = true;
        return;
    }
    const long long q = __double2ll_rn(v * scale);
    if (q != 0) atomicAdd(&s_sum[c], (unsigned long long)q);
}

// rule 5 for one sum
__device__ __forceinline__ double pool_mean(unsigned long long s, double len, double unscale) {
    return (__ll2double_rn((long long)s) / len) * unscale;
}

template <typename T, bool CSR>
__global__ __launch_bounds__(kPoolThreads) void k_neighbor_pool(
    const T* __restrict__ val, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t ld, int64_t n,
    int32_t W, const int64_t* __restrict__ g_indptr, const int32_t* __restrict__ g_indices, uint32_t n_tiles, int shift,
    const int32_t* __restrict__ n_cells, double* __restrict__ out, int64_t ldo, int32_t* __restrict__ flags) {
    __shared__ unsigned long long s_sum[kPoolTile];
    const int64_t i = (int64_t)(blockIdx.x / n_tiles);
    const int32_t c0 = (int32_t)(blockIdx.x % n_tiles) * kPoolTile;
    const int32_t width = W - c0 < kPoolTile ? W - c0 : kPoolTile;
    for (int k = threadIdx.x; k < width; k += kPoolThreads) s_sum[k] = 0;
    __syncthreads();

    constexpr int RL = kPoolRowLanes;
    static_assert(RL >= 4 && 64 % RL == 0, "the head and the tail of a dense row take up to 3 lanes of a group");
    const int lane = threadIdx.x % RL, group = threadIdx.x / RL;
    const double scale = pb_pow2(shift);
    const int64_t g0 = g_indptr[i];
    const int64_t positions = g_indptr[i + 1] - g0 + 1;  // the cell, then its graph row
    bool nonfinite = false, bad_column = false;
    for (int64_t p = group; p < positions; p += kPoolThreads / RL) {
        int64_t r = i;
        if (p > 0) {
            r = g_indices[g0 + p - 1];
            if (r == i) continue;  // (an explicit diagonal entry: the cell is position 0)
            if (r < 0 || r >= n) {
                bad_column = true;  // never dereferenced
                continue;
            }
        }
        if (CSR) {
            const int64_t e1 = indptr[r + 1];
            for (int64_t e = indptr[r] + lane; e < e1; e += RL) {
                const int64_t c = (int64_t)indices[e] - c0;
                if (c >= 0 && c < width) pool_add((double)val[e], (int)c, scale, s_sum, nonfinite);
            }
        } else {
            constexpr int V = 16 / (int)sizeof(T);  // values per 16-byte load
            const T* q = val + r * ld + c0;
            // the values in front of the first 16-byte boundary, at most V - 1 (q is a multiple of sizeof(T))
            int head = (int)(((16 - (reinterpret_cast<uintptr_t>(q) & 15)) & 15) / sizeof(T));
            head = head < width ? head : width;
            const int n_vec = (width - head) / V;
            if (lane < head) pool_add((double)q[lane], lane, scale, s_sum, nonfinite);
            for (int k = lane; k < n_vec; k += RL) {
                const int c = head + k * V;
                alignas(16) T v[V];
                *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(q + c);
#pragma unroll
                for (int j = 0; j < V; ++j) pool_add((double)v[j], c + j, scale, s_sum, nonfinite);
            }
            const int c = head + n_vec * V + lane;  // the values behind the last whole load, at most V - 1
            if (lane < V && c < width) pool_add((double)q[c], c, scale, s_sum, nonfinite);
        }
    }
    __syncthreads();

    const int32_t cells = n_cells[i];
    const double len = (double)(cells > 0 ? cells : 1), unscale = pb_pow2(-shift);
    double* o = out + i * ldo + c0;
    int head = (int)((reinterpret_cast<uintptr_t>(o) >> 3) & 1);  // one float64 in front of the 16-byte boundary, or none
    head = head < width ? head : width;
    const int n_pairs = (width - head) / 2;
    if (threadIdx.x == 0 && head) o[0] = pool_mean(s_sum[0], len, unscale);
    for (int k = threadIdx.x; k < n_pairs; k += kPoolThreads) {
        const int c = head + 2 * k;
        double2 m;
        m.x = pool_mean(s_sum[c], len, unscale);
        m.y = pool_mean(s_sum[c + 1], len, unscale);
        *reinterpret_cast<double2*>(o + c) = m;
    }
    const int last = head + 2 * n_pairs;
    if (threadIdx.x == kPoolThreads - 1 && last < width) o[last] = pool_mean(s_sum[last], len, unscale);
    const int f = (nonfinite ? kPoolFlagNonfinite : 0) | (bad_column ? kPoolFlagColumn : 0);
    if (f) atomicOr(flags, f);
}

}  // namespace icv

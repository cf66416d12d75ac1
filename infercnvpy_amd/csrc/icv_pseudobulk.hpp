// tl.cnv_pseudobulk: the mean profile of every group of cells, exactly.  The contract
// (tests/_pseudobulk_oracle.py restates it):
//   1. stored values are used as float64 (a float32 is promoted exactly); an entry that is not stored is 0.
//   2. shift e in [0, 40]; every stored magnitude is < 2^10 (the caller's check), so |v 2^e| < 2^50.
//   3. q = rint(v 2^e), ties to even, as int64 (the product is exact: a power of two).
//   4. S[g,w] = the int64 sum of q over the listed rows of group g; N[g,w] = the int32 number of stored values != 0 among
//      them.  -0.0 and a stored 0.0 add to neither.  Integer adds: the order does not matter.
//   5. mean = (double(S) / double(L_g)) 2^-e with L_g the number of listed rows: one round-to-nearest-even conversion, one
//      correctly rounded division, an exact scaling; fraction = double(N) / double(L_g).  L_g = 0 gives 0 / 0.
//
// Geometry of rules 1-4: the listed rows of every group are cut into slabs of kPbSlab positions (a slab never crosses a
// group boundary; slab_off[g] = the slabs of the groups before g, a prefix sum of ceil(L_g / kPbSlab)), the windows into
// tiles of kPbTile.  One workgroup per (slab, tile) keeps the tile's int64 sums and int32 counts in LDS (12 bytes per
// window, 48 KB), one wavefront takes one row at a time, lanes stride the row's stored entries (CSR) or its windows (dense,
// 16-byte loads from the first 16-byte boundary of the row's tile on) and add into LDS with LDS atomics.  At the end the
// accumulators that are not 0 go to global memory with one integer atomic each: one per (slab, window), never one per
// entry.  No floating-point sum anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_graph.hpp"

namespace icv {

constexpr int kPbTile = 4096;     // windows per workgroup: 12 bytes of LDS each
constexpr int kPbSlab = 128;      // listed rows per workgroup
constexpr int kPbThreads = 512;   // 8 wavefronts, 16 rows each in a full slab
constexpr int kPbMaxShift = 40;
constexpr int kPbFlagNonfinite = 1, kPbFlagRow = 2;

// 2^k as a float64 for -1022 <= k <= 1023
__device__ __forceinline__ double pb_pow2(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }

// positions [lo, hi) of group g in `rows`, inside [0, M] whatever group_ptr holds
__device__ __forceinline__ void pb_group_span(const int64_t* __restrict__ group_ptr, int64_t g, int64_t M, int64_t& lo,
                                              int64_t& hi) {
    lo = group_ptr[g];
    hi = group_ptr[g + 1];
    lo = lo < 0 ? 0 : (lo > M ? M : lo);
    hi = hi < lo ? lo : (hi > M ? M : hi);
}

// slabs[g] = ceil(L_g / kPbSlab)
__global__ __launch_bounds__(256) void k_pb_slab_counts(const int64_t* __restrict__ group_ptr, int64_t G, int64_t M,
                                                        int64_t* __restrict__ slabs) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    int64_t lo, hi;
    pb_group_span(group_ptr, g, M, lo, hi);
    slabs[g] = (hi - lo + kPbSlab - 1) / kPbSlab;
}

// rule 3 and the two adds of rule 4 for one value of window column c of the tile
__device__ __forceinline__ void pb_add(double v, int c, double scale, unsigned long long* s_sum, int* s_cnt, bool& nonfinite) {
    if (v == 0.0) return;  // (0.0 and -0.0; NaN goes on)
    if (!(__builtin_fabs(v) < __builtin_inf())) {
        nonfinite = true;
        return;
    }
    atomicAdd(&s_cnt[c], 1);
    const long long q = __double2ll_rn(v * scale);
    if (q != 0) atomicAdd(&s_sum[c], (unsigned long long)q);
}

template <typename T, bool CSR>
__global__ __launch_bounds__(kPbThreads) void k_group_profiles(
    const T* __restrict__ val, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t ld,
    int64_t n_rows, int32_t W, const int64_t* __restrict__ rows, int64_t M, const int64_t* __restrict__ group_ptr, int64_t G,
    const int64_t* __restrict__ slab_off, uint32_t n_tiles, int shift, unsigned long long* __restrict__ sum,
    int32_t* __restrict__ stored, int32_t* __restrict__ flags) {
    __shared__ unsigned long long s_sum[kPbTile];
    __shared__ int s_cnt[kPbTile];
    const int64_t slab = (int64_t)(blockIdx.x / n_tiles);
    if (slab >= slab_off[G]) return;  // (the grid is an upper bound of the slabs; the whole workgroup leaves)
    const int32_t c0 = (int32_t)(blockIdx.x % n_tiles) * kPbTile;
    const int32_t width = W - c0 < kPbTile ? W - c0 : kPbTile;
    const int64_t g = last_group_at(slab_off, G, slab);  // the group of this slab
    int64_t lo, hi;
    pb_group_span(group_ptr, g, M, lo, hi);
    const int64_t pos0 = lo + (slab - slab_off[g]) * kPbSlab;
    const int64_t pos1 = pos0 + kPbSlab < hi ? pos0 + kPbSlab : hi;

    for (int i = threadIdx.x; i < width; i += kPbThreads) {
        s_sum[i] = 0;
        s_cnt[i] = 0;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double scale = pb_pow2(shift);
    bool nonfinite = false, bad_row = false;
    for (int64_t pos = pos0 + wave; pos < pos1; pos += kPbThreads / 64) {
        const int64_t r = rows[pos];
        if (r < 0 || r >= n_rows) {
            bad_row = true;
            continue;
        }
        if (CSR) {
            const int64_t e1 = indptr[r + 1];
            for (int64_t e = indptr[r] + lane; e < e1; e += 64) {
                const int64_t c = (int64_t)indices[e] - c0;
                if (c >= 0 && c < width) pb_add((double)val[e], (int)c, scale, s_sum, s_cnt, nonfinite);
            }
        } else {
            constexpr int V = 16 / (int)sizeof(T);  // values per 16-byte load
            const T* p = val + r * ld + c0;
            // the values in front of the first 16-byte boundary, at most V - 1 (p is a multiple of sizeof(T))
            int head = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
            head = head < width ? head : width;
            const int n_vec = (width - head) / V;
            if (lane < head) pb_add((double)p[lane], lane, scale, s_sum, s_cnt, nonfinite);
            for (int k = lane; k < n_vec; k += 64) {
                const int c = head + k * V;
                alignas(16) T v[V];
                *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(p + c);
#pragma unroll
                for (int j = 0; j < V; ++j) pb_add((double)v[j], c + j, scale, s_sum, s_cnt, nonfinite);
            }
            const int c = head + n_vec * V + lane;  // the values behind the last whole load, at most V - 1
            if (lane < V && c < width) pb_add((double)p[c], c, scale, s_sum, s_cnt, nonfinite);
        }
    }
    __syncthreads();

    unsigned long long* gs = sum + g * (int64_t)W + c0;
    int32_t* gn = stored + g * (int64_t)W + c0;
    for (int i = threadIdx.x; i < width; i += kPbThreads) {
        const unsigned long long s = s_sum[i];
        const int n = s_cnt[i];
        if (s) atomicAdd(gs + i, s);
        if (n) atomicAdd(gn + i, n);
    }
    const int f = (nonfinite ? kPbFlagNonfinite : 0) | (bad_row ? kPbFlagRow : 0);
    if (f) atomicOr(flags, f);
}

// rule 5, one thread per group and window
__global__ __launch_bounds__(256) void k_group_profiles_finish(const int64_t* __restrict__ sum, const int32_t* __restrict__ stored,
                                                               const int64_t* __restrict__ group_ptr, int64_t G, int32_t W,
                                                               int shift, double* __restrict__ mean,
                                                               double* __restrict__ fraction) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= G * (int64_t)W) return;
    const int64_t g = k / W;
    const int64_t L = group_ptr[g + 1] - group_ptr[g];
    double m = 0.0, f = 0.0;
    if (L > 0) {
        const double len = __ll2double_rn(L);
        m = (__ll2double_rn(sum[k]) / len) * pb_pow2(-shift);
        f = (double)stored[k] / len;
    }
    mean[k] = m;
    fraction[k] = f;
}

}  // namespace icv

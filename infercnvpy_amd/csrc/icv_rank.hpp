// tl.cnv_rank_groups: the doubled mid-rank sums of every group in every window, exactly.  The contract
// (tests/_rank_oracle.py restates it):
//   1. an entry that is not stored is 0, a stored 0.0 or -0.0 is the same 0, a float32 is used as the float64 it converts
//      to; a value that is not finite raises bit 0 of the flag word and is ranked nowhere.
//   2. the population is the rows with code >= 0, N of them (N < 2^21: N^3 fits an int64).  For a cell with value x in
//      window w, 2r = #{x_j < x} + #{x_j <= x} + 1 over the population; R2[g,w] = the int64 sum of 2r over the cells with
//      code g, T[w] = the int64 sum over the distinct values of c^3 - c with c the number of cells that have the value.
//
// Geometry: (a) k_rank_count counts per window the population's stored values that are not 0 (LDS counters per window tile
// and slab of rows, one wavefront per row, one integer atomic per (slab, window)).  The caller cuts the windows into
// consecutive tiles whose entries fit its workspace and runs (b)-(d) per tile.  (b) k_rank_scatter writes every such value
// of the tile to its window's segment as (key, code): key is the order-preserving uint64 image of the float64, the slots
// come from integer atomics on the window's cursor, so the order inside a segment is arbitrary and nothing below
// depends on it.  (c) every segment is sorted by key.  (d) k_rank_sums: with s and e the first position of an entry's run
// of equal keys and the position behind it, counted from the segment's start, and z0 = N - (the segment's length) the size
// of the zero block, 2r = s + e + 1 for a negative value and s + e + 1 + 2 z0 for a positive one.  s and e are p and p + 1
// where the neighbours differ and come from a binary search for the lower and the upper bound in the sorted segment
// otherwise: a run has any length and lies anywhere, no tile, wavefront or workgroup boundary exists for it.  The sums are
// integer adds (LDS per group up to kRkLdsGroups codes, 64-bit global atomics beyond), c^3 - c is added by the run's first
// entry.  (e) k_rank_finish adds the zero block: R2 += (n_g - cnt_g)(2 neg + z0 + 1), T += z0^3 - z0.  Integer adds only:
// the tables do not depend on the order of execution.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icv {

constexpr int kRkTile = 8192;        // windows per workgroup of the count: 4 bytes of LDS each
constexpr int kRkSlab = 128;         // rows per workgroup of the count and the scatter
constexpr int kRkThreads = 512;      // 8 wavefronts, 16 rows each
constexpr int kRkSumThreads = 256;   // threads of a workgroup of the rank sums
constexpr int kRkChunk = 2048;       // sorted entries per workgroup of the rank sums: 8 per thread
constexpr int kRkLdsGroups = 2048;   // codes whose sums a workgroup keeps in LDS: 12 bytes each
constexpr int64_t kRkMaxCells = 1ll << 21;  // N below this: N^3 fits an int64
constexpr int kRkFlagNonfinite = 1;
constexpr unsigned long long kRkSign = 0x8000000000000000ull;

// the order-preserving image of a finite float64 that is not 0: a < b as doubles  <=>  rk_key(a) < rk_key(b) as uint64;
// a negative value lies below kRkSign, a positive one above
__device__ __forceinline__ unsigned long long rk_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b & kRkSign) ? ~b : (b | kRkSign);
}

// 0: the value is 0 (either sign), 1: it is ranked, 2: it is not finite
__device__ __forceinline__ int rk_kind(double v) {
    if (v == 0.0) return 0;
    return __builtin_fabs(v) < __builtin_inf() ? 1 : 2;
}

// f(c, v) for every stored value of row r with a window number c0 + c, 0 <= c < width, by the 64 lanes of one wavefront:
// lanes stride the row's stored entries (CSR; columns in any order) or its windows (dense, 16-byte loads from the first
// 16-byte boundary of the row's tile on)
template <typename T, bool CSR, typename F>
__device__ __forceinline__ void rk_visit_row(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                             const int32_t* __restrict__ indices, int64_t ld, int64_t r, int32_t c0, int32_t width,
                                             int lane, F&& f) {
    if (CSR) {
        const int64_t e1 = indptr[r + 1];
        for (int64_t e = indptr[r] + lane; e < e1; e += 64) {
            const int64_t c = (int64_t)indices[e] - c0;
            if (c >= 0 && c < width) f((int)c, (double)val[e]);
        }
    } else {
        constexpr int V = 16 / (int)sizeof(T);  // values per 16-byte load
        const T* p = val + r * ld + c0;
        // the values in front of the first 16-byte boundary, at most V - 1 (p is a multiple of sizeof(T))
        int head = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
        head = head < width ? head : width;
        const int n_vec = (width - head) / V;
        if (lane < head) f(lane, (double)p[lane]);
        for (int k = lane; k < n_vec; k += 64) {
            const int c = head + k * V;
            alignas(16) T v[V];
            *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(p + c);
#pragma unroll
            for (int j = 0; j < V; ++j) f(c + j, (double)v[j]);
        }
        const int c = head + n_vec * V + lane;  // the values behind the last whole load, at most V - 1
        if (lane < V && c < width) f(c, (double)p[c]);
    }
}

// (a) stored[w] += the rows of the slab with code >= 0 whose value at w is ranked; grid = slabs x tiles
template <typename T, bool CSR>
__global__ __launch_bounds__(kRkThreads) void k_rank_count(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices, int64_t ld, int64_t n_rows,
                                                           int32_t W, const int32_t* __restrict__ code, uint32_t n_tiles,
                                                           int32_t* __restrict__ stored, int32_t* __restrict__ flags) {
    __shared__ int s_cnt[kRkTile];
    const int64_t row0 = (int64_t)(blockIdx.x / n_tiles) * kRkSlab;
    const int64_t row1 = row0 + kRkSlab < n_rows ? row0 + kRkSlab : n_rows;
    const int32_t c0 = (int32_t)(blockIdx.x % n_tiles) * kRkTile;
    const int32_t width = W - c0 < kRkTile ? W - c0 : kRkTile;
    for (int i = threadIdx.x; i < width; i += kRkThreads) s_cnt[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool nonfinite = false;
    for (int64_t r = row0 + wave; r < row1; r += kRkThreads / 64) {
        if (code[r] < 0) continue;
        rk_visit_row<T, CSR>(val, indptr, indices, ld, r, c0, width, lane, [&](int c, double v) {
            const int kind = rk_kind(v);
            if (kind == 1) atomicAdd(&s_cnt[c], 1);
            if (kind == 2) nonfinite = true;
        });
    }
    __syncthreads();
    for (int i = threadIdx.x; i < width; i += kRkThreads) {
        const int n = s_cnt[i];
        if (n) atomicAdd(stored + c0 + i, n);
    }
    if (nonfinite) atomicOr(flags, kRkFlagNonfinite);
}

// (b) the ranked values of the windows [w0, w0 + n_win) of the population's rows, as (key, code) pairs in their window's
// segment [seg_off[c], seg_off[c + 1]); cursor (n_win, zeroed) hands the slots out.  grid = slabs x tiles of kRkTile
// windows.  The workgroup counts its slab's values per window in LDS as k_rank_count does, takes a range of every window's
// segment with ONE integer atomic per (slab, window) and hands the slots of its range out with LDS atomics in a second pass
// over the same rows (a global atomic with a return value per value is what a one-pass form waits for).  A slot outside
// the segment (the matrix is not the one that was counted) is not written.
template <typename T, bool CSR>
__global__ __launch_bounds__(kRkThreads) void k_rank_scatter(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                             const int32_t* __restrict__ indices, int64_t ld, int64_t n_rows,
                                                             const int32_t* __restrict__ code, int32_t w0, int32_t n_win,
                                                             uint32_t n_tiles, const int32_t* __restrict__ seg_off,
                                                             int32_t* __restrict__ cursor, unsigned long long* __restrict__ keys,
                                                             int32_t* __restrict__ payload) {
    __shared__ int s_pos[kRkTile];
    const int64_t row0 = (int64_t)(blockIdx.x / n_tiles) * kRkSlab;
    const int64_t row1 = row0 + kRkSlab < n_rows ? row0 + kRkSlab : n_rows;
    const int32_t t0 = (int32_t)(blockIdx.x % n_tiles) * kRkTile;  // the tile's first window, counted from w0
    const int32_t width = n_win - t0 < kRkTile ? n_win - t0 : kRkTile;
    for (int i = threadIdx.x; i < width; i += kRkThreads) s_pos[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = row0 + wave; r < row1; r += kRkThreads / 64) {
        if (code[r] < 0) continue;
        rk_visit_row<T, CSR>(val, indptr, indices, ld, r, w0 + t0, width, lane, [&](int c, double v) {
            if (rk_kind(v) == 1) atomicAdd(&s_pos[c], 1);
        });
    }
    __syncthreads();
    for (int i = threadIdx.x; i < width; i += kRkThreads) {
        const int n = s_pos[i];
        s_pos[i] = n ? atomicAdd(&cursor[t0 + i], n) : 0;  // the first slot of this workgroup's range
    }
    __syncthreads();
    for (int64_t r = row0 + wave; r < row1; r += kRkThreads / 64) {
        const int32_t g = code[r];
        if (g < 0) continue;
        rk_visit_row<T, CSR>(val, indptr, indices, ld, r, w0 + t0, width, lane, [&](int c, double v) {
            if (rk_kind(v) != 1) return;
            const int32_t b = seg_off[t0 + c], len = seg_off[t0 + c + 1] - b;
            const int32_t slot = atomicAdd(&s_pos[c], 1);
            if (slot >= 0 && slot < len) {
                keys[(int64_t)b + slot] = rk_key(v);
                payload[(int64_t)b + slot] = g;
            }
        });
    }
}

// the first position in [lo, hi) of the ascending k whose key is not below key (hi if none)
__device__ __forceinline__ int32_t rk_lower_bound(const unsigned long long* __restrict__ k, int32_t lo, int32_t hi,
                                                  unsigned long long key) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the first position in [lo, hi) of the ascending k whose key is above key (hi if none)
__device__ __forceinline__ int32_t rk_upper_bound(const unsigned long long* __restrict__ k, int32_t lo, int32_t hi,
                                                  unsigned long long key) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// (d) grid = (n_win, chunks of the longest segment): the workgroup takes the sorted entries [chunk kRkChunk, + kRkChunk) of
// window w0 + blockIdx.x and adds 2r to r2[code, w], 1 to cnt[code, w], c^3 - c to tie[w] at the first entry of a run of
// c > 1 and its negatives to neg[w].  r2 and cnt are n_codes x W tables; a code outside [0, n_codes) adds nothing.  LDS:
// the sums of the workgroup per code in LDS, then one global atomic per code that occurred; else global atomics per entry.
template <bool LDS>
__global__ __launch_bounds__(kRkSumThreads) void k_rank_sums(const unsigned long long* __restrict__ keys,
                                                             const int32_t* __restrict__ payload,
                                                             const int32_t* __restrict__ seg_off, int32_t w0, int32_t W,
                                                             int64_t n_pop, int32_t n_codes, unsigned long long* __restrict__ r2,
                                                             int32_t* __restrict__ cnt, unsigned long long* __restrict__ tie,
                                                             int32_t* __restrict__ neg) {
    __shared__ unsigned long long s_r2[LDS ? kRkLdsGroups : 1];
    __shared__ int s_cnt[LDS ? kRkLdsGroups : 1];
    __shared__ int s_neg;
    const int32_t b = seg_off[blockIdx.x], len = seg_off[blockIdx.x + 1] - b;
    const int32_t p0 = (int32_t)blockIdx.y * kRkChunk;
    if (p0 >= len) return;  // (the grid covers the longest segment; the whole workgroup leaves)
    const int32_t p1 = p0 + kRkChunk < len ? p0 + kRkChunk : len;
    const int64_t w = (int64_t)w0 + blockIdx.x;
    const unsigned long long* k = keys + b;
    const int32_t* pay = payload + b;
    if (LDS)
        for (int i = threadIdx.x; i < n_codes; i += kRkSumThreads) {
            s_r2[i] = 0;
            s_cnt[i] = 0;
        }
    if (threadIdx.x == 0) s_neg = 0;
    __syncthreads();

    const unsigned long long z2 = 2ull * (unsigned long long)(n_pop - len);  // 2 z0
    int negatives = 0;
    for (int32_t p = p0 + threadIdx.x; p < p1; p += kRkSumThreads) {
        const unsigned long long key = k[p];
        const int32_t s = (p > 0 && k[p - 1] == key) ? rk_lower_bound(k, 0, p - 1, key) : p;
        const int32_t e = (p + 1 < len && k[p + 1] == key) ? rk_upper_bound(k, p + 2, len, key) : p + 1;
        unsigned long long two_r = (unsigned long long)s + (unsigned long long)e + 1ull;
        if (key < kRkSign) ++negatives; else two_r += z2;
        const int32_t g = pay[p];
        if (g >= 0 && g < n_codes) {
            if (LDS) {
                atomicAdd(&s_r2[g], two_r);
                atomicAdd(&s_cnt[g], 1);
            } else {
                atomicAdd(r2 + (int64_t)g * W + w, two_r);
                atomicAdd(cnt + (int64_t)g * W + w, 1);
            }
        }
        if (p == s && e - s > 1) {
            const unsigned long long c = (unsigned long long)(e - s);
            atomicAdd(tie + w, c * c * c - c);
        }
    }
    if (negatives) atomicAdd(&s_neg, negatives);
    __syncthreads();
    if (LDS)
        for (int i = threadIdx.x; i < n_codes; i += kRkSumThreads) {
            const int n = s_cnt[i];
            if (n) {
                atomicAdd(r2 + (int64_t)i * W + w, s_r2[i]);
                atomicAdd(cnt + (int64_t)i * W + w, n);
            }
        }
    if (threadIdx.x == 0 && s_neg) atomicAdd(neg + w, s_neg);
}

// (e) the zero block, one thread per (g, w) of the n_groups tested groups: z0 = n_pop - stored[w] cells share the doubled
// rank 2 neg[w] + z0 + 1, and n_cells[g] - cnt[g,w] of them are of group g; the thread of group 0 adds z0^3 - z0 to tie[w]
__global__ __launch_bounds__(256) void k_rank_finish(const int32_t* __restrict__ stored, const int32_t* __restrict__ neg,
                                                     const int32_t* __restrict__ cnt, const int64_t* __restrict__ n_cells,
                                                     int64_t n_groups, int32_t W, int64_t n_pop, int64_t* __restrict__ r2,
                                                     int64_t* __restrict__ tie) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_groups * (int64_t)W) return;
    const int64_t g = i / W, w = i % W;
    const int64_t z0 = n_pop - stored[w];
    r2[i] += (n_cells[g] - cnt[i]) * (2 * (int64_t)neg[w] + z0 + 1);
    if (g == 0) tie[w] += z0 * z0 * z0 - z0;
}

}  // namespace icv

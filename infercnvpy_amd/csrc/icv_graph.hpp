// What tl.leiden, tl.umap and tl.tsne share on the device: the counter hash, the wavefront sum,
// the row length above which a row takes a workgroup, and the validation of a stored entry of the symmetric CSR graph.
// Also the search of a group table that tl.cnv_segments and tl.cnv_pseudobulk share (last_group_at).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icv {

constexpr int kGraphLongRow = 512;  // longest row a wavefront stages in LDS (kLdLdsRow = kUmLdsRow = kTsLongRow)

__host__ __device__ __forceinline__ uint64_t ld_mix(uint64_t z) {  // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ long long ld_wave_sum(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The last g in [0, G) with ptr[g] <= pos, for an ascending ptr with ptr[0] <= pos: the group that holds position pos of a
// list sorted by group (groups of no entries before it share its offset and are passed over).  0 when G < 2.
__device__ __forceinline__ int64_t last_group_at(const int64_t* __restrict__ ptr, int64_t G, int64_t pos) {
    int64_t glo = 0, ghi = G;
    while (ghi - glo > 1) {
        const int64_t mid = glo + (ghi - glo) / 2;
        if (ptr[mid] <= pos) glo = mid;
        else ghi = mid;
    }
    return glo;
}

// The flags of stored entry i (value x = (float)val[i]) of row v, whose entries start at b: 1 non-finite, 2 negative,
// 4 diagonal, 8 column out of range, 16 row not strictly ascending, 32 not symmetric (row c is searched for column v
// and the values are compared as floats).
template <typename T>
__device__ __forceinline__ unsigned graph_entry_flags(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                      const T* __restrict__ val, int64_t n, int64_t v, int64_t b, int64_t i,
                                                      float x) {
    const int64_t c = col[i];
    unsigned f = 0;
    if (!(fabsf(x) <= 3.4028234663852886e38f)) f |= 1;
    else if (x < 0.f) f |= 2;
    if (c == v) f |= 4;
    if (i > b && col[i - 1] >= c) f |= 16;
    if (c < 0 || c >= n) {
        f |= 8;
    } else {
        int64_t l = indptr[c], r = indptr[c + 1];
        while (l < r) {
            const int64_t m = (l + r) >> 1;
            if (col[m] < v) l = m + 1;
            else r = m;
        }
        if (!(l < indptr[c + 1] && col[l] == v && (float)val[l] == x)) f |= 32;
    }
    return f;
}

// *p = max(*p, v).  The word only grows, so a row that reads a value >= its own (even a stale one) has nothing to add:
// the atomics of all rows go to one address and are what the validation kernel waits for.
__device__ __forceinline__ void graph_raise(unsigned* p, unsigned v) {
    if (v > __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMax(p, v);
}

// Validation of tl.umap and tl.tsne (a wavefront per row).  head[0] flags, head[1] number of long rows (listed in
// long_list, any order), head[2] bits of the largest finite non-negative weight (-0.0 counts as 0; non-negative floats
// order as unsigned), head[3] longest row (saturated at 2^31 - 1)
__global__ __launch_bounds__(256) void k_graph_check(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                     const float* __restrict__ val, int64_t n, unsigned* __restrict__ head,
                                                     int32_t* __restrict__ long_list) {
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n) return;
    const int64_t b = indptr[v], e = indptr[v + 1];
    unsigned f = 0, top = 0;
    for (int64_t i = b + lane; i < e; i += 64) {
        const float x = val[i];
        const unsigned fe = graph_entry_flags(indptr, col, val, n, v, b, i, x);
        if (!(fe & 3)) top = max(top, __float_as_uint(x == 0.f ? 0.f : x));
        f |= fe;
    }
    for (int off = 32; off > 0; off >>= 1) {
        f |= __shfl_xor(f, off, 64);
        top = max(top, (unsigned)__shfl_xor(top, off, 64));
    }
    if (lane == 0) {
        const int64_t len = e - b;
        if (f) atomicOr(&head[0], f);
        graph_raise(&head[2], top);
        graph_raise(&head[3], (unsigned)(len > 0x7fffffff ? 0x7fffffff : len));
        if (len > kGraphLongRow) long_list[atomicAdd(&head[1], 1u)] = (int32_t)v;
    }
}

}  // namespace icv

// pp.neighbors: exact k nearest neighbours of n points in d <= 256 dimensions and UMAP's fuzzy graph.
//
//   k_knn_colsum / k_knn_mean / k_knn_center   column-centred float32 copies Z (rows padded to DP floats), the scaled
//                                               norms s_i = (1 - c) |z_i|^2 and the largest |z_i|^2
//   k_knn_candidates<NK>                        fp32 MFMA sweep: per row the L smallest keys
//                                                   key(i, j) = s_i + s_j - 2 z_i.z_j  <=  d2(i, j)      (lower bounds)
//                                               of each part of the columns; the n x n tile never leaves the registers
//   k_knn_rerank                                rule 2 in float64 for the candidates, rule 3 order, the certificate
//   k_knn_exact                                 the uncertified rows against all n cells in float64
//   k_knn_rowsum / k_knn_total / k_knn_smooth   rho, sigma, membership strengths
//   k_knn_sym_count / k_knn_sym_fill / k_knn_sort_rows   C = A + A^T - A o A^T as canonical CSR
//
// Key and certificate.  With u = 2^-24 and A = |z_i|^2 + |z_j|^2 (exact norms of the float32 copies):
//   * z = fl(x - mu) componentwise, so x_i - x_j = z_i - z_j + e with |e| <= u' (|z_i| + |z_j|):
//     d2 >= |z_i - z_j|^2 - 4.0001 u A                        (any mu: the bound does not need the exact mean)
//   * the MFMA chain of DP products: |dot^ - dot| <= gamma A / 2, gamma = (DP + 2) u / (1 - (DP + 2) u)
//   * s^ = fl32((1 - c) |z|^2), fl(s^_i + s^_j) <= (1 - c) A (1 + u)^3; the last subtraction adds <= 2.01 u A
//   so key^ <= d2 - (c - gamma - 9.03 u) A: c = (DP + 16) u makes every computed key a lower bound of the exact
//   squared distance, up to 1e-30 absolute for underflow (flushed subnormal operands and products).  A candidate list
//   keeps the L smallest keys of its columns; every column it dropped has key >= the list's largest kept key, so
//   T_i = min over the row's lists of that value bounds the distance of every cell that is not a candidate.  The row
//   is certified when T_i - 1e-30 > exact d2 of its (k-1)-th neighbour, and the bound is only trusted while
//   max |z|^2 < 1e36 (no overflow anywhere above); otherwise the row is listed for k_knn_exact.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "icv_corr.hpp"

namespace icv {

constexpr int kKnnSlack = 8;        // list length L = k - 1 + kKnnSlack
constexpr int kKnnRows = 128;       // query rows per workgroup of k_knn_candidates (4 wavefronts x 32)
constexpr int kKnnMaxParts = 16;    // column parts (second grid dimension)
constexpr double kKnnAbs = 1e-30;   // underflow allowance of the key
constexpr float kKnnMaxNorm = 1e36f;

// partial[b * d + c] = float64 sum of column c over the rows of slab b (rows_per rows each), row order
__global__ void __launch_bounds__(256) k_knn_colsum(const float* __restrict__ x, int64_t n, int d, int64_t ld,
                                                    int64_t rows_per, double* __restrict__ partial) {
    const int c = threadIdx.x;
    if (c >= d) return;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) s += (double)x[r * ld + c];
    partial[(int64_t)blockIdx.x * d + c] = s;
}

// mu[c] = float32(sum of the slabs' partial sums, slab order / n); maxbits = 0
__global__ void __launch_bounds__(256) k_knn_mean(const double* __restrict__ partial, int n_slabs, int d, int64_t n,
                                                  float* __restrict__ mu, unsigned* __restrict__ maxbits) {
    const int c = threadIdx.x;
    if (c == 0) *maxbits = 0u;
    if (c >= d) return;
    double s = 0.0;
    for (int b = 0; b < n_slabs; ++b) s += partial[(int64_t)b * d + c];
    mu[c] = (float)(s / (double)n);
}

// z[i][c] = fl32(x[i][c] - mu[c]) (c < d; zero up to dp; rows n .. n_pad zero), snorm[i] = fl32((1 - cfac) |z_i|^2),
// maxbits = max over i of the bits of fl32(|z_i|^2) (non-negative floats order as their bits: an integer maximum)
__global__ void __launch_bounds__(256) k_knn_center(const float* __restrict__ x, int64_t n, int64_t n_pad, int d, int64_t ld,
                                                    int dp, const float* __restrict__ mu, double cfac,
                                                    float* __restrict__ z, float* __restrict__ snorm,
                                                    unsigned* __restrict__ maxbits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    float* zr = z + i * dp;
    if (i >= n) {
        for (int c = 0; c < dp; ++c) zr[c] = 0.0f;
        snorm[i] = 0.0f;
        return;
    }
    double q = 0.0;
    for (int c = 0; c < d; ++c) {
        const float v = x[i * ld + c] - mu[c];
        zr[c] = v;
        q += (double)v * (double)v;
    }
    for (int c = d; c < dp; ++c) zr[c] = 0.0f;
    snorm[i] = (float)((1.0 - cfac) * q);
    atomicMax(maxbits, __float_as_uint((float)q));
}

// Candidate sweep.  Workgroup = 4 wavefronts; wavefront w owns the 32 query rows q0 = 128 blockIdx.x + 32 w .. + 31 and
// keeps their operand (B of v_mfma_f32_32x32x2_f32: column = lane & 31) in NK float4 registers per lane for the whole
// sweep.  Column part blockIdx.y covers the candidates [part * chunk, (part + 1) * chunk), 32 per tile (operand A:
// row = lane & 31), read straight from global memory (the four wavefronts of a workgroup and the workgroups of an XCD
// sweep the same tiles at the same time: L1 / L2 hits).  As in k_gram_mfma a lane reads four consecutive K values with
// one 16-byte load, the lower half-wavefront K = 8 g .. 8 g + 3, the upper 8 g + 4 .. 8 g + 7.
// Result layout D: column (query) = lane & 31, row (candidate) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): lane and
// lane + 32 share a query and see disjoint candidates, so EVERY LANE keeps its own list of the L smallest keys in LDS
// (keys[slot][lane]: conflict free), unsorted, with the largest kept key and its slot in registers: a tile value is
// compared with one register, and only a smaller one costs a replace + a scan of the L slots.
// Output: cand[(q * parts + part) * 2 L + half * L + slot] = candidate index (-1: empty slot),
//         bound[(q * parts + part) * 2 + half] = largest kept key (+inf while the list is not full).
template <int NK>
__global__ void __launch_bounds__(256) k_knn_candidates(const float* __restrict__ z, const float* __restrict__ snorm,
                                                        int64_t n, int64_t n_pad, int64_t chunk, int L,
                                                        int32_t* __restrict__ cand, float* __restrict__ bound) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    constexpr int DP = NK * 8;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5;
    float* keys = reinterpret_cast<float*>(knn_lds) + (size_t)wave * 2 * L * 64;
    int32_t* idx = reinterpret_cast<int32_t*>(keys + (size_t)L * 64);
    const int64_t q = (int64_t)blockIdx.x * kKnnRows + wave * 32 + (lane & 31);  // < n_pad (grid covers n_pad / 128 ... see host)
    const int parts = gridDim.y, part = blockIdx.y;
    const int64_t j_begin = (int64_t)part * chunk;
    int64_t j_end = j_begin + chunk;
    if (j_end > n_pad) j_end = n_pad;

    const float inf = __builtin_huge_valf();
    for (int s = 0; s < L; ++s) {
        keys[s * 64 + lane] = inf;
        idx[s * 64 + lane] = -1;
    }
    float worst = inf;
    int wslot = 0;

    const bool q_ok = q < n_pad;
    const int64_t qq = q_ok ? q : 0;
    float4 bq[NK];
    const float4* zq = reinterpret_cast<const float4*>(z + qq * DP) + half;
#pragma unroll
    for (int g = 0; g < NK; ++g) bq[g] = zq[2 * g];
    const float sq = snorm[qq];

    for (int64_t j0 = j_begin; j0 < j_end; j0 += 32) {  // j0 + 31 < n_pad (n_pad and chunk are multiples of 32)
        const float4* za = reinterpret_cast<const float4*>(z + (j0 + (lane & 31)) * DP) + half;
        float4 a[NK];
#pragma unroll
        for (int g = 0; g < NK; ++g) a[g] = za[2 * g];
        float4 sj[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) sj[r4] = *reinterpret_cast<const float4*>(snorm + j0 + 8 * r4 + 4 * half);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int g = 0; g < NK; ++g) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].x, bq[g].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].y, bq[g].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].z, bq[g].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].w, bq[g].w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float4 s4 = sj[r >> 2];
            const float sjr = (r & 3) == 0 ? s4.x : (r & 3) == 1 ? s4.y : (r & 3) == 2 ? s4.z : s4.w;
            const float key = (sq + sjr) - 2.0f * acc[r];
            const int64_t j = j0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (key < worst && j < n && j != q) {
                keys[wslot * 64 + lane] = key;
                idx[wslot * 64 + lane] = (int32_t)j;
                float w = -inf;
                int ws = 0;
                for (int s = 0; s < L; ++s) {
                    const float kk = keys[s * 64 + lane];
                    if (kk > w) {
                        w = kk;
                        ws = s;
                    }
                }
                worst = w;
                wslot = ws;
            }
        }
    }
    if (q < n) {
        const int64_t base = (q * parts + part) * 2;
        int32_t* co = cand + base * L + (int64_t)half * L;
        for (int s = 0; s < L; ++s) co[s] = idx[s * 64 + lane];
        bound[base + half] = worst;
    }
}

// lexicographic (d2, j) comparison of rule 3
__device__ __forceinline__ bool knn_less(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }

// rule 2: float64 sum over the columns in order, no fused multiply-add (-ffp-contract=off)
__device__ __forceinline__ double knn_d2(const float* __restrict__ a, const float* __restrict__ b, int d) {
    double s = 0.0;
    for (int c = 0; c < d; ++c) {
        const double t = (double)a[c] - (double)b[c];
        s += t * t;
    }
    return s;
}

// the wavefront's smallest (d2, j) (all lanes get it); j = INT_MAX: none
__device__ __forceinline__ void knn_wave_min(double& dv, int& jv) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(dv, off, 64);
        const int oj = __shfl_xor(jv, off, 64);
        if (knn_less(od, oj, dv, jv)) {
            dv = od;
            jv = oj;
        }
    }
}

// One wavefront per row: exact d2 of the row's m = parts * 2 L candidates from the ORIGINAL points, the first k - 1 in
// (d2, j) order, the certificate.  Uncertified rows are appended to redo[] (integer counter; the ORDER of that list
// does not reach any result).  LDS: m (8 + 4) bytes.
__global__ void __launch_bounds__(64) k_knn_rerank(const float* __restrict__ x, int64_t n, int d, int64_t ld,
                                                   const int32_t* __restrict__ cand, const float* __restrict__ bound,
                                                   int parts, int L, int km1, const unsigned* __restrict__ maxbits,
                                                   int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                   int32_t* __restrict__ redo, unsigned* __restrict__ n_redo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    const int m = parts * 2 * L, lane = threadIdx.x;
    double* dd = reinterpret_cast<double*>(knn_lds);
    int32_t* jj = reinterpret_cast<int32_t*>(dd + m);
    const int64_t i = blockIdx.x;
    const float* xi = x + i * ld;
    const int32_t* ci = cand + i * m;
    for (int e = lane; e < m; e += 64) {
        const int32_t j = ci[e];
        jj[e] = j;
        dd[e] = j >= 0 ? knn_d2(xi, x + (int64_t)j * ld, d) : 0.0;
    }
    __syncthreads();
    double t_min = (double)__builtin_huge_valf();
    for (int e = lane; e < parts * 2; e += 64) {
        const double b = (double)bound[i * parts * 2 + e];
        t_min = b < t_min ? b : t_min;  // (a NaN bound cannot occur below kKnnMaxNorm)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(t_min, off, 64);
        t_min = o < t_min ? o : t_min;
    }
    double last_d = -1.0;
    int last_j = -1;
    bool full = true;
    for (int r = 0; r < km1; ++r) {
        double bd = (double)__builtin_huge_valf();
        int bj = 0x7fffffff;
        for (int e = lane; e < m; e += 64) {
            const int j = jj[e];
            if (j < 0) continue;
            const double v = dd[e];
            if (knn_less(last_d, last_j, v, j) && knn_less(v, j, bd, bj)) {
                bd = v;
                bj = j;
            }
        }
        knn_wave_min(bd, bj);
        if (bj == 0x7fffffff) {
            full = false;
            break;
        }
        if (lane == 0) {
            out_idx[i * km1 + r] = bj;
            out_dist[i * km1 + r] = (float)sqrt(bd);
        }
        last_d = bd;
        last_j = bj;
    }
    const bool certified = full && __uint_as_float(*maxbits) < kKnnMaxNorm && t_min - kKnnAbs > last_d;
    if (!certified && lane == 0) redo[atomicAdd(n_redo, 1u)] = (int32_t)i;
}

// One workgroup per listed row: rule 2 against all n cells, k - 1 rounds of "smallest (d2, j) after the previous one".
__global__ void __launch_bounds__(256) k_knn_exact(const float* __restrict__ x, int64_t n, int d, int64_t ld, int km1,
                                                   const int32_t* __restrict__ redo, int32_t* __restrict__ out_idx,
                                                   float* __restrict__ out_dist) {
    __shared__ double sd[4];
    __shared__ int sj[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = redo[blockIdx.x];
    const float* xi = x + i * ld;
    double last_d = -1.0;
    int last_j = -1;
    for (int r = 0; r < km1; ++r) {
        double bd = (double)__builtin_huge_valf();
        int bj = 0x7fffffff;
        for (int64_t j = t; j < n; j += 256) {
            if (j == i) continue;
            const double v = knn_d2(xi, x + j * ld, d);
            if (knn_less(last_d, last_j, v, (int)j) && knn_less(v, (int)j, bd, bj)) {
                bd = v;
                bj = (int)j;
            }
        }
        knn_wave_min(bd, bj);
        __syncthreads();  // sd / sj of the previous round are read
        if (lane == 0) {
            sd[wave] = bd;
            sj[wave] = bj;
        }
        __syncthreads();
        bd = sd[0];
        bj = sj[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (knn_less(sd[w], sj[w], bd, bj)) {
                bd = sd[w];
                bj = sj[w];
            }
        if (t == 0) {
            out_idx[i * km1 + r] = bj;
            out_dist[i * km1 + r] = (float)sqrt(bd);
        }
        last_d = bd;
        last_j = bj;
    }
}

// ---- fuzzy graph ---------------------------------------------------------------------------------------------------
// rowsum[i] = float64 sum of the row's stored distances, in order
__global__ void __launch_bounds__(256) k_knn_rowsum(const float* __restrict__ dist, int64_t n, int km1,
                                                    double* __restrict__ rowsum) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int r = 0; r < km1; ++r) s += (double)dist[i * km1 + r];
    rowsum[i] = s;
}

// total[0] = sum of rowsum in a fixed order: thread t the elements t, t + 1024, ..., then a tree over the threads
__global__ void __launch_bounds__(1024) k_knn_total(const double* __restrict__ rowsum, int64_t n, double* __restrict__ total) {
    __shared__ double sh[1024];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = t; i < n; i += 1024) s += rowsum[i];
    sh[t] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    if (t == 0) total[0] = sh[0];
}

// One lane per row: rho, UMAP's bisection for sigma, the membership strengths (all float64; DESIGN.md 4.9 rule 5)
__global__ void __launch_bounds__(256) k_knn_smooth(const float* __restrict__ dist, int64_t n, int km1,
                                                    const double* __restrict__ rowsum, const double* __restrict__ total,
                                                    double* __restrict__ rho_out, double* __restrict__ sigma_out,
                                                    double* __restrict__ w_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* dr = dist + i * km1;
    double rho = 0.0;
    for (int r = 0; r < km1; ++r)
        if (dr[r] > 0.0f) {  // the row is ascending: the first positive one is the smallest
            rho = (double)dr[r];
            break;
        }
    const double target = log2((double)(km1 + 1));
    double lo = 0.0, hi = (double)__builtin_huge_valf(), mid = 1.0;
    const double inf = hi;
    for (int it = 0; it < 64; ++it) {
        double s = 0.0;
        for (int r = 0; r < km1; ++r) {
            const double g = (double)dr[r] - rho;
            s += exp(-((g > 0.0 ? g : 0.0) / mid));
        }
        if (fabs(s - target) < 1e-5) break;
        if (s > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == inf ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double floor_v = rho > 0.0 ? 1e-3 * (rowsum[i] / (double)km1) : 1e-3 * (total[0] / ((double)n * (double)km1));
    const double sigma = mid < floor_v ? floor_v : mid;
    rho_out[i] = rho;
    sigma_out[i] = sigma;
    for (int r = 0; r < km1; ++r) {
        const double g = (double)dr[r] - rho;
        w_out[i * km1 + r] = g <= 0.0 ? 1.0 : exp(-(g / sigma));
    }
}

// value of C at (i, idx[i][s]) and whether row j = idx[i][s] lists i.  SUM = false: the fuzzy union A + A^T - A o A^T
// (pp.neighbors); SUM = true: A + A^T (tl.tsne, DESIGN.md 4.12 rule 3)
template <bool SUM>
__device__ __forceinline__ float knn_sym_value(const int32_t* __restrict__ idx, const double* __restrict__ w, int km1,
                                               int64_t i, int s, int& j, bool& mutual) {
    j = idx[i * km1 + s];
    const double wij = w[i * km1 + s];
    double wji = 0.0;
    mutual = false;
    const int32_t* rj = idx + (int64_t)j * km1;
    for (int r = 0; r < km1; ++r)
        if (rj[r] == (int32_t)i) {
            wji = w[(int64_t)j * km1 + r];
            mutual = true;
            break;
        }
    return SUM ? (float)(wij + wji) : (float)((wij + wji) - wij * wji);
}

// count[r] += stored entries of row r of C: its own neighbours, and the rows that list r without being listed by it
// (integer atomics: the counts do not depend on the order).  Entries that round to 0 in float32 are not stored.
template <bool SUM>
__global__ void __launch_bounds__(256) k_knn_sym_count(const int32_t* __restrict__ idx, const double* __restrict__ w,
                                                       int64_t n, int km1, unsigned long long* __restrict__ count) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * km1) return;
    const int64_t i = e / km1;
    int j;
    bool mutual;
    const float c = knn_sym_value<SUM>(idx, w, km1, i, (int)(e - i * km1), j, mutual);
    if (c == 0.0f) return;
    atomicAdd(count + i, 1ull);
    if (!mutual) atomicAdd(count + j, 1ull);
}

// the same walk, writing (column, value) at indptr[row] + cursor[row]++ (any order: k_knn_sort_rows makes it canonical)
template <bool SUM>
__global__ void __launch_bounds__(256) k_knn_sym_fill(const int32_t* __restrict__ idx, const double* __restrict__ w,
                                                      int64_t n, int km1, const int64_t* __restrict__ indptr,
                                                      unsigned* __restrict__ cursor, int32_t* __restrict__ cols,
                                                      float* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * km1) return;
    const int64_t i = e / km1;
    int j;
    bool mutual;
    const float c = knn_sym_value<SUM>(idx, w, km1, i, (int)(e - i * km1), j, mutual);
    if (c == 0.0f) return;
    int64_t p = indptr[i] + atomicAdd(cursor + i, 1u);
    cols[p] = j;
    vals[p] = c;
    if (!mutual) {
        p = indptr[j] + atomicAdd(cursor + j, 1u);
        cols[p] = (int32_t)i;
        vals[p] = c;
    }
}

// One wavefront per row: the row's (column, value) pairs by ascending column (columns of a row are distinct: the rank
// of an entry is the number of smaller columns).
__global__ void __launch_bounds__(256) k_knn_sort_rows(const int64_t* __restrict__ indptr, int64_t n,
                                                       const int32_t* __restrict__ cols_in, const float* __restrict__ vals_in,
                                                       int32_t* __restrict__ cols, float* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const int64_t b = indptr[i], m = indptr[i + 1] - b;
    for (int64_t e = lane; e < m; e += 64) {
        const int32_t c = cols_in[b + e];
        int64_t rank = 0;
        for (int64_t f = 0; f < m; ++f) rank += cols_in[b + f] < c;
        cols[b + rank] = c;
        vals[b + rank] = vals_in[b + e];
    }
}

}  // namespace icv

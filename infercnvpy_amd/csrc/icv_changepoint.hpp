// tl.cnv_changepoints: the exact penalised least-squares segmentation (optimal partitioning, L2 cost) of
// every chromosome of every row.  The contract (tests/_changepoint_oracle.py restates it), for one row and one chromosome
// with the values x_1 .. x_L (an entry that is not stored is 0.0), the penalty beta >= 0 and the shortest segment m >= 1:
//   1. P_0 = Q_0 = +0.0, P_j = P_{j-1} + x_j, Q_j = Q_{j-1} + x_j x_j, ascending and sequential.
//   2. cost of the segment (i, j]: d = P_j - P_i, c = (Q_j - Q_i) - (d d) / (double)(j - i), c < 0.0 becomes 0.0.
//   3. F_0 = 0.0, F_j = min over the admissible i of ((F_i + c(i, j)) + beta); i is admissible when (i == 0 or i >= m) and
//      j - i >= m, and i = 0 always is for j = L; a j without an admissible i has F_j = +inf and is never chosen.  The
//      minimum is the smallest value, ties go to the lowest i: a total order on (value, i).
//   4. backtrack from L; the segment (i, j] has the level (P_j - P_i) / (double)(j - i).
//   5. levels = the level of the window's segment, starts = 1 at the first window of every segment.
// Only float64 adds, multiplies, divisions and compares in the written order; the library is built -ffp-contract=off and
// the division is the correctly rounded one, so the kernel equals the oracle bit for bit.
//
// Geometry: one wavefront (a 64-thread workgroup) per (row, chromosome).  The work is quadratic in L, and a block needs LDS
// for its own chromosome alone: P, Q, F as L + 1 doubles each and the back-pointers as L + 1 int32, 28 (L + 1) bytes; the
// values lie where F_1 .. F_L go (they are dead once the chains of rule 1 are formed) and the backtrack's list of segment
// starts where F lay.  kCpMaxChrWindows keeps one chromosome inside a CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icv {

constexpr int kCpMaxChrWindows = 4096;  // = ICV_CHANGEPOINT_MAX_CHR_WINDOWS: 28 x 4097 = 112 KiB of the CU's 160 KiB
constexpr int kCpLdsPerWindow = 28;     // P, Q, F (float64) and the back-pointer (int32)

// the dynamic LDS of a call whose longest chromosome has `longest` windows
inline size_t cp_lds_bytes(int32_t longest) { return ((size_t)(longest + 1) * kCpLdsPerWindow + 15) / 16 * 16; }

// the windows [s0, s1) of chromosome c, clamped to [0, W] and to `cap` windows (the host checked both: with the clamps no
// LDS access leaves the block's arrays whatever chr_start holds); false when it has none
__device__ __forceinline__ bool cp_chr(const int32_t* __restrict__ chr_start, int32_t c, int32_t W, int32_t cap, int32_t& s0,
                                       int32_t& s1) {
    s0 = min(max(chr_start[c], 0), W), s1 = min(max(chr_start[c + 1], 0), W);
    if (s1 - s0 > cap) s1 = s0 + cap;
    return s1 > s0;
}

// the values of the windows [s0, s1) of one row into x[0, L); ends with a barrier.  CSR columns need not be sorted.
template <typename T, bool CSR>
__device__ __forceinline__ void cp_load_chr(double* x, int32_t s0, int32_t s1, const T* val, const int64_t* indptr,
                                            const int32_t* indices, int64_t ld, int64_t row, int lane) {
    const int32_t L = s1 - s0;
    if (CSR) {
        for (int32_t t = lane; t < L; t += 64) x[t] = 0.0;
        __syncthreads();
        const int64_t b = indptr[row], e = indptr[row + 1];
        for (int64_t k = b + lane; k < e; k += 64) {
            const int32_t c = indices[k];
            if (c >= s0 && c < s1) x[c - s0] = (double)val[k];
        }
    } else {
        const T* src = val + row * ld + s0;
        for (int32_t t = lane; t < L; t += 64) x[t] = (double)src[t];
    }
    __syncthreads();
}

// One step of a wavefront-wide minimum through the data-parallel primitives (no LDS traffic): every lane combines its value
// with the one `CTRL` names; a lane that CTRL or ROW_MASK leaves out gets its own value back and keeps it.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int cp_dpp(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double cp_min_step(double v) {
    const int lo = cp_dpp<CTRL, ROW_MASK>(__double2loint(v)), hi = cp_dpp<CTRL, ROW_MASK>(__double2hiint(v));
    const double o = __hiloint2double(hi, lo);
    return o < v ? o : v;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int32_t cp_min_step(int32_t v) {
    const int32_t o = cp_dpp<CTRL, ROW_MASK>(v);
    return o < v ? o : v;
}
// The smallest v of the 64 lanes, in every lane: shifts by 1, 2, 4 and 8 lanes leave the minimum of each row of 16 in its
// last lane, lane 15 of rows 0 and 2 goes to rows 1 and 3, lane 31 to rows 2 and 3, and lane 63 holds the whole.  A minimum
// is the same in whatever order it is formed.
template <typename V>
__device__ __forceinline__ V cp_wave_min_last(V v) {
    v = cp_min_step<0x111, 0xf>(v);  // row_shr:1
    v = cp_min_step<0x112, 0xf>(v);  // row_shr:2
    v = cp_min_step<0x114, 0xf>(v);  // row_shr:4
    v = cp_min_step<0x118, 0xf>(v);  // row_shr:8
    v = cp_min_step<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v = cp_min_step<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ double cp_wave_min(double v) {
    v = cp_wave_min_last(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ int32_t cp_wave_min(int32_t v) { return __builtin_amdgcn_readlane(cp_wave_min_last(v), 63); }

// ---- rules 1-5: one wavefront per (row, chromosome); cap = the windows the launch's LDS holds ------------------------------
template <typename T, bool CSR>
__global__ __launch_bounds__(64) void k_changepoint_levels(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                           const int32_t* __restrict__ chr_start, int32_t C, int32_t cap,
                                                           double beta, int32_t m, double* __restrict__ levels,
                                                           uint8_t* __restrict__ starts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cp_lds[];
    const int lane = threadIdx.x;
    const int64_t row = (int64_t)(blockIdx.x / (uint32_t)C);
    const int32_t chr = (int32_t)(blockIdx.x % (uint32_t)C);
    int32_t s0, s1;
    if (!cp_chr(chr_start, chr, W, cap, s0, s1)) return;
    const int32_t L = s1 - s0;
    double* P = reinterpret_cast<double*>(cp_lds);
    double* Q = P + (L + 1);
    double* F = Q + (L + 1);
    int32_t* back = reinterpret_cast<int32_t*>(F + (L + 1));
    double* x = F + 1;

    cp_load_chr<T, CSR>(x, s0, s1, val, indptr, indices, ld, row, lane);

    // rule 1: lane 0 chains P, lane 1 chains Q
    if (lane < 2) {
        double* chain = lane == 0 ? P : Q;
        double acc = 0.0;
        chain[0] = acc;
        for (int32_t t = 0; t < L; ++t) {
            const double v = x[t];
            acc = acc + (lane == 0 ? v : v * v);
            chain[t + 1] = acc;
        }
    }
    __syncthreads();
    if (lane == 0) F[0] = 0.0, back[0] = 0;
    __syncthreads();

    // rules 2-3
    const double inf = __builtin_huge_val();
    for (int32_t j = 1; j <= L; ++j) {
        const double Pj = P[j], Qj = Q[j];
        double best = inf;
        int32_t bi = 0x7fffffff;
        // the admissible i, numbered k = 0, 1, ...: i = 0 (where it counts), then m .. j - m; a lane's k ascend, and so do
        // its i, so the strict < keeps the lowest i of equal values
        const bool with_zero = j >= m || j == L;
        const int32_t n_cand = 1 + max(j - 2 * m + 1, 0);
        for (int32_t k = lane + (with_zero ? 0 : 64 * (lane == 0)); k < n_cand; k += 64) {
            const int32_t i = k == 0 ? 0 : m + k - 1;
            const double d = Pj - P[i];
            double c = (Qj - Q[i]) - (d * d) / (double)(j - i);
            if (c < 0.0) c = 0.0;
            const double v = (F[i] + c) + beta;
            if (v < best) best = v, bi = i;
        }
        // the smallest value of the wavefront, then the lowest i among the lanes that hold it: the total order of rule 3
        const double least = cp_wave_min(best);
        const int32_t who = cp_wave_min(best == least ? bi : 0x7fffffff);
        if (lane == 0) F[j] = least, back[j] = who == 0x7fffffff ? 0 : who;
        __syncthreads();
    }

    // rule 4: one lane lists the segment starts from the last segment to the first, at most L of them whatever back holds;
    // the list takes F's place
    int32_t* seg = reinterpret_cast<int32_t*>(F);
    int32_t* n_seg = seg + L;  // (F has room for 2 (L + 1) int32)
    __syncthreads();
    if (lane == 0) {
        int32_t k = 0;
        for (int32_t j = L; j > 0 && k < L; ++k) {
            int32_t i = back[j];
            if (i < 0 || i >= j) i = 0;
            seg[k] = i;
            j = i;
        }
        *n_seg = k;
    }
    __syncthreads();

    // rule 5
    const int32_t K = *n_seg;
    double* out = levels + row * (int64_t)W + s0;
    uint8_t* first = starts + row * (int64_t)W + s0;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t i = seg[k], j = k == 0 ? L : seg[k - 1];
        const double level = (P[j] - P[i]) / (double)(j - i);
        for (int32_t t = i + lane; t < j; t += 64) out[t] = level, first[t] = (uint8_t)(t == i);
    }
}

// ---- rule 6: e[row, c] = the chain, from +0.0, of (x_{t+1} - x_t)^2 over the adjacent windows of chromosome c ---------------
// x: L doubles and sq: L doubles of LDS (16 bytes per window)
template <typename T, bool CSR>
__global__ __launch_bounds__(64) void k_changepoint_diffsq(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                           const int32_t* __restrict__ chr_start, int32_t C, int32_t cap,
                                                           double* __restrict__ e) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cp_lds[];
    const int lane = threadIdx.x;
    const int64_t row = (int64_t)(blockIdx.x / (uint32_t)C);
    const int32_t chr = (int32_t)(blockIdx.x % (uint32_t)C);
    int32_t s0, s1;
    if (!cp_chr(chr_start, chr, W, cap, s0, s1)) {
        if (lane == 0) e[blockIdx.x] = 0.0;
        return;
    }
    const int32_t L = s1 - s0;
    double* x = reinterpret_cast<double*>(cp_lds);
    double* sq = x + L;
    cp_load_chr<T, CSR>(x, s0, s1, val, indptr, indices, ld, row, lane);
    for (int32_t t = lane; t + 1 < L; t += 64) {
        const double d = x[t + 1] - x[t];
        sq[t] = d * d;
    }
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;
        for (int32_t t = 0; t + 1 < L; ++t) acc = acc + sq[t];
        e[blockIdx.x] = acc;
    }
}

// d[row] = the sum, from +0.0, of e[row, c] over the chromosomes in ascending order: one thread per row
__global__ __launch_bounds__(256) void k_changepoint_rowsum(const double* __restrict__ e, int64_t n_rows, int32_t C,
                                                            double* __restrict__ d) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const double* src = e + r * (int64_t)C;
    double acc = 0.0;
    for (int32_t c = 0; c < C; ++c) acc = acc + src[c];
    d[r] = acc;
}

}  // namespace icv

// tl.cnv_states: per-cell loss / neutral / gain calls of X_cnv by a three-state Viterbi chain along
// every chromosome.  The contract (tests/_states_oracle.py restates it):
//   1. host scalars, passed as doubles: h = 1.0 / (2.0 sigma sigma), stay = log(1 - p), sw = log(p / 2); the default
//      sigma = sqrt(S / (n W)), S = fsum on the host of the per-row sums q_i of k_states_rowsq (v v over the row's stored
//      entries in stored order, one sequential float64 sum per row); the default amplitude a = 2 sigma.
//   2. emission of state s in {0, 1, 2} with means (-a, 0.0, +a): t = x - mu_s, e_s = -(t t) h.
//   3. chain over the windows of one chromosome: d_0(s) = e_s(x_0); d_t(s) = best_r(d_{t-1}(r) + T(r, s)) + e_s(x_t),
//      T = stay for r = s and sw otherwise; best = the largest value, ties to r = s first, then to the lower r.
//   4. the last window takes the s with the largest d, ties to neutral, then loss, then gain; then backtrack.
//   5. output = state - 1.  An entry that is not stored is 0.0.  Chains never cross a chromosome boundary.
// Only float64 adds, multiplies and compares in a fixed order; the library is built -ffp-contract=off, so the
// expressions below are evaluated as written and the kernel equals the oracle bit for bit.
//
// Geometry: that of icv_hmm.hpp (one wavefront per cell, the row as W doubles in LDS, lane c running the chromosomes
// c, c + 64, ...); the back-pointers (2 bits x 3 states) take one LDS byte per window, which the backtrack overwrites
// with the state.  9 bytes of LDS per window and resident cell; ICV_STATES_MAX_WINDOWS keeps one cell inside a CU's
// 160 KiB.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_hmm.hpp"  // hmm_load_row, hmm_chr

namespace icv {

constexpr int kStMaxWindows = 16384;  // = ICV_STATES_MAX_WINDOWS: 9 x 16384 = 144 KiB of the CU's 160 KiB
constexpr int kStLdsPerWindow = 9;    // the float64 value + the back-pointer byte

inline size_t st_lds_bytes(int32_t n_windows) { return ((size_t)n_windows * kStLdsPerWindow + 15) / 16 * 16; }

// ---- rule 1: q_i = sum of v v over row i's stored entries, one lane per row, in stored order ----------------------------
// *bad is set when a value is not finite (the caller zeroes it)
template <typename T>
__global__ __launch_bounds__(256) void k_states_rowsq_csr(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                          int64_t n_rows, double* __restrict__ q, int32_t* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t b = indptr[r], e = indptr[r + 1];
    double s = 0.0;
    bool nf = false;
    for (int64_t k = b; k < e; ++k) {
        const double v = (double)val[k];
        nf |= !(fabs(v) <= 1.7976931348623157e308);
        s = s + v * v;
    }
    q[r] = s;
    if (nf) atomicOr(bad, 1);
}

// a dense row: every element is a stored entry (a zero adds +0.0, so the sum equals the CSR one bit for bit)
template <typename T>
__global__ __launch_bounds__(256) void k_states_rowsq_dense(const T* __restrict__ x, int64_t ld, int64_t n_rows,
                                                            int32_t n_cols, double* __restrict__ q,
                                                            int32_t* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const T* row = x + r * ld;
    double s = 0.0;
    bool nf = false;
    for (int32_t j = 0; j < n_cols; ++j) {
        const double v = (double)row[j];
        nf |= !(fabs(v) <= 1.7976931348623157e308);
        s = s + v * v;
    }
    q[r] = s;
    if (nf) atomicOr(bad, 1);
}

// the share of a row's windows that are not neutral: the exact count over W, one correctly rounded float64 division
__global__ __launch_bounds__(256) void k_states_fraction(const int32_t* __restrict__ count, int64_t n_rows, int32_t W,
                                                         double* __restrict__ fraction) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n_rows) fraction[r] = (double)count[r] / (double)W;
}

struct StParams {
    double a, h, stay, sw;
};

// rule 2 for the three states
__device__ __forceinline__ void st_emit(double x, const StParams& P, double& e0, double& e1, double& e2) {
    const double t0 = x - (-P.a), t1 = x - 0.0, t2 = x - P.a;
    e0 = -(t0 * t0) * P.h;
    e1 = -(t1 * t1) * P.h;
    e2 = -(t2 * t2) * P.h;
}

// ---- rules 2-5: one wavefront per cell (chr_start: see hmm_chr) -----------------------------------------------------------
template <typename T, bool CSR>
__global__ __launch_bounds__(64) void k_states_viterbi(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                       const int32_t* __restrict__ chr_start, int32_t C, StParams P,
                                                       int8_t* __restrict__ states, int32_t* __restrict__ nonneutral) {
    extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
    double* x = reinterpret_cast<double*>(st_lds);
    unsigned char* bp = st_lds + (size_t)W * sizeof(double);
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;

    for (int32_t j = lane; j < W; j += 64) bp[j] = 1;  // (a window no chromosome covers stays neutral)
    hmm_load_row<T, CSR>(x, W, val, indptr, indices, ld, row, lane);

    int32_t count = 0;
    for (int32_t c = lane; c < C; c += 64) {
        int32_t s0, s1;
        if (!hmm_chr(chr_start, c, W, s0, s1)) continue;
        double d0, d1, d2;
        st_emit(x[s0], P, d0, d1, d2);
        for (int32_t t = s0 + 1; t < s1; ++t) {
            double e0, e1, e2;
            st_emit(x[t], P, e0, e1, e2);
            const double k0 = d0 + P.stay, k1 = d1 + P.stay, k2 = d2 + P.stay;  // r = s
            const double w0 = d0 + P.sw, w1 = d1 + P.sw, w2 = d2 + P.sw;        // r != s
            // r = s first, then the other two in ascending r; only a strictly larger value replaces
            double b0 = k0, b1 = k1, b2 = k2;
            unsigned a0 = 0, a1 = 1, a2 = 2;
            if (w1 > b0) b0 = w1, a0 = 1;
            if (w2 > b0) b0 = w2, a0 = 2;
            if (w0 > b1) b1 = w0, a1 = 0;
            if (w2 > b1) b1 = w2, a1 = 2;
            if (w0 > b2) b2 = w0, a2 = 0;
            if (w1 > b2) b2 = w1, a2 = 1;
            d0 = b0 + e0, d1 = b1 + e1, d2 = b2 + e2;
            bp[t] = (unsigned char)(a0 | (a1 << 2) | (a2 << 4));
        }
        // rule 4: neutral, then loss, then gain
        unsigned s = 1;
        double best = d1;
        if (d0 > best) best = d0, s = 0;
        if (d2 > best) best = d2, s = 2;
        for (int32_t t = s1 - 1; t > s0; --t) {
            const unsigned back = bp[t];
            bp[t] = (unsigned char)s;
            count += s != 1;
            s = (back >> (2 * s)) & 3u;
        }
        bp[s0] = (unsigned char)s;
        count += s != 1;
    }
    __syncthreads();

    // rule 5, the row written in 4-byte words where the output is aligned (single bytes before and after)
    int8_t* out = states + row * (int64_t)W;
    const int32_t head = min(W, (int32_t)((4 - (reinterpret_cast<uintptr_t>(out) & 3)) & 3));
    const int32_t n_words = (W - head) >> 2;
    if (lane < head) out[lane] = (int8_t)((int)bp[lane] - 1);
    uint32_t* out4 = reinterpret_cast<uint32_t*>(out + head);
    for (int32_t k = lane; k < n_words; k += 64) {
        const unsigned char* p = bp + head + 4 * k;
        const uint32_t v0 = (uint8_t)(p[0] - 1), v1 = (uint8_t)(p[1] - 1), v2 = (uint8_t)(p[2] - 1), v3 = (uint8_t)(p[3] - 1);
        out4[k] = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
    }
    const int32_t tail = head + 4 * n_words + lane;
    if (lane < 3 && tail < W) out[tail] = (int8_t)((int)bp[tail] - 1);

    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
    if (lane == 0) nonneutral[row] = count;
}

}  // namespace icv

// tl.cnv_copy_states: per-cell copy-number calls of X_cnv by a K-state Viterbi chain, 2 <= K <= 8, along
// every chromosome.  The contract (tests/_copy_states_oracle.py restates it):
//   1. host scalars, passed as doubles: h = 1.0 / (2.0 sigma sigma), stay = log(1 - p), sw = log(p / (K - 1)); the state
//      means mu_0 < ... < mu_{K-1} with mu_z = 0.0 (z: the neutral state) are passed by value.
//   2. emission of state s: t = x - mu_s, e_s = -(t t) h.  An entry that is not stored is 0.0.
//   3. chain over the windows of one chromosome: d_0(s) = e_s(x_0); d_t(s) = best_r(d_{t-1}(r) + T(r, s)) + e_s(x_t),
//      T = stay for r = s and sw otherwise; best = the largest value, ties to r = s first, then to the lowest r.
//   4. the last window takes the s with the largest d, tried in the order z, z - 1, z + 1, z - 2, z + 2, ...; only a
//      strictly larger value replaces; then backtrack.
//   5. output = s - z.  Chains never cross a chromosome boundary; a window that no chromosome covers is 0.
// Only float64 adds, multiplies and compares in a fixed order; the library is built -ffp-contract=off, so the expressions
// below are evaluated as written and the kernel equals the oracle bit for bit.  With the means (-a, 0.0, a) the rules are
// those of icv_states.hpp and so are the bytes.
//
// Rule 3 in O(K): every transition that leaves a state costs the same sw, so all states share the candidates
// w_r = d(r) + sw.  Let a1 be the first r with the largest w_r and a2 the first r != a1 with the largest w_r among those.
// Among the r != s, tried in ascending order with only a strictly larger value replacing, the winner is a1 for every
// s != a1 and a2 for s = a1: state s compares d(s) + stay with w_a1 (or w_a2), and the K^2 form does nothing else.
//
// Geometry: that of icv_hmm.hpp (one wavefront per cell, the row as W doubles in LDS, lane c running the chromosomes
// c, c + 64, ...).  d, e and the means stay in registers: K is a template parameter, every loop over the states is
// unrolled and no array is indexed by a run-time value.  A window's back-pointers are one 16-bit LDS word: bit s set when
// state s stayed (K <= 8 bits), a1 in bits 8-10 and a2 in bits 11-13; the backtrack overwrites the word with the state.
// 10 bytes of LDS per window and resident cell; ICV_COPY_STATES_MAX_WINDOWS keeps one cell inside a CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_hmm.hpp"  // hmm_load_row, hmm_chr

namespace icv {

constexpr int kCsMaxStates = 8;        // K <= 8: the "stayed" mask is the low byte of the back-pointer word
constexpr int kCsMaxWindows = 16384;   // = ICV_COPY_STATES_MAX_WINDOWS: 10 x 16384 = 160 KiB, the CU's LDS
constexpr int kCsLdsPerWindow = 10;    // the float64 value + the 16-bit back-pointer word

inline size_t cs_lds_bytes(int32_t n_windows) { return ((size_t)n_windows * kCsLdsPerWindow + 15) / 16 * 16; }

// the model of the K-state kernels: k_copy_states_viterbi and the forward-backward kernels of icv_copy_posterior.hpp
struct CsParams {
    double mu[kCsMaxStates];  // the first K are used
    double h;
    double stay, sw;  // a step that stays / leaves for one other state: log(1 - p), log(p / (K - 1)) for Viterbi,
                      // the probabilities ps = 1 - p, pw = p / (K - 1) for forward-backward
    int32_t z;  // the neutral state: mu[z] == 0.0
};

// rule 2 for the K states
template <int K>
__device__ __forceinline__ void cs_emit(double x, const CsParams& P, double (&e)[K]) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const double t = x - P.mu[s];
        e[s] = -(t * t) * P.h;
    }
}

// one int8 row of W calls written in 4-byte words where the output is aligned (single bytes before and after);
// f(word) is the byte of a window from its LDS word
template <typename F>
__device__ __forceinline__ void cs_write_plane(int8_t* out, const uint16_t* bp, int32_t W, int lane, F f) {
    const int32_t head = min(W, (int32_t)((4 - (reinterpret_cast<uintptr_t>(out) & 3)) & 3));
    const int32_t n_words = (W - head) >> 2;
    if (lane < head) out[lane] = (int8_t)f(bp[lane]);
    uint32_t* out4 = reinterpret_cast<uint32_t*>(out + head);
    for (int32_t k = lane; k < n_words; k += 64) {
        const uint16_t* p = bp + head + 4 * k;
        const uint32_t v0 = (uint8_t)f(p[0]), v1 = (uint8_t)f(p[1]), v2 = (uint8_t)f(p[2]), v3 = (uint8_t)f(p[3]);
        out4[k] = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
    }
    const int32_t tail = head + 4 * n_words + lane;
    if (lane < 3 && tail < W) out[tail] = (int8_t)f(bp[tail]);
}

// ---- rules 2-5: one wavefront per cell (chr_start: see hmm_chr) -----------------------------------------------------------
// states: s - z; sign: the same clipped to -1 / 0 / +1; nonneutral: the row's count of s != z
template <typename T, bool CSR, int K>
__global__ __launch_bounds__(64) void k_copy_states_viterbi(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                            const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                            const int32_t* __restrict__ chr_start, int32_t C, CsParams P,
                                                            int8_t* __restrict__ states, int8_t* __restrict__ sign,
                                                            int32_t* __restrict__ nonneutral) {
    static_assert(K >= 2 && K <= kCsMaxStates, "the stayed mask has 8 bits, a1 and a2 three each");
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
    double* x = reinterpret_cast<double*>(cs_lds);
    uint16_t* bp = reinterpret_cast<uint16_t*>(cs_lds + (size_t)W * sizeof(double));
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const unsigned z = (unsigned)P.z;

    for (int32_t j = lane; j < W; j += 64) bp[j] = (uint16_t)z;  // (a window no chromosome covers stays neutral)
    hmm_load_row<T, CSR>(x, W, val, indptr, indices, ld, row, lane);

    int32_t count = 0;
    for (int32_t c = lane; c < C; c += 64) {
        int32_t s0, s1;
        if (!hmm_chr(chr_start, c, W, s0, s1)) continue;
        double d[K];
        cs_emit<K>(x[s0], P, d);
        for (int32_t t = s0 + 1; t < s1; ++t) {
            double e[K];
            cs_emit<K>(x[t], P, e);
            // a1, a2 of w_r = d(r) + sw: ascending r, only a strictly larger value replaces
            double m1 = d[0] + P.sw, m2 = d[1] + P.sw;
            unsigned a1 = 0, a2 = 1;
            if (m2 > m1) {
                const double w = m1;
                m1 = m2, m2 = w, a1 = 1, a2 = 0;
            }
#pragma unroll
            for (int r = 2; r < K; ++r) {
                const double w = d[r] + P.sw;
                if (w > m1)
                    m2 = m1, a2 = a1, m1 = w, a1 = r;
                else if (w > m2)
                    m2 = w, a2 = r;
            }
            // r = s first, then the best of the others
            unsigned word = (a1 << 8) | (a2 << 11);
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const double keep = d[s] + P.stay;
                const double other = a1 == (unsigned)s ? m2 : m1;
                const bool left = other > keep;
                d[s] = (left ? other : keep) + e[s];
                word |= left ? 0u : 1u << s;
            }
            bp[t] = (uint16_t)word;
        }
        // rule 4: the largest d; among equal ones the first of z, z - 1, z + 1, z - 2, ... (its place in that order is
        // 2 |s - z| - (s < z))
        unsigned s = 0;
        double best = d[0];
        int place = 2 * (int)z;  // (s = 0: z places below or at z; for z = 0 it is the first)
        if (z > 0) place -= 1;
#pragma unroll
        for (int r = 1; r < K; ++r) {
            const int dist = r - (int)z;
            const int pr = dist < 0 ? -2 * dist - 1 : 2 * dist;
            if (d[r] > best || (d[r] == best && pr < place)) best = d[r], s = r, place = pr;
        }
        for (int32_t t = s1 - 1; t > s0; --t) {
            const unsigned back = bp[t];
            bp[t] = (uint16_t)s;
            count += s != z;
            if (!((back >> s) & 1u)) {
                const unsigned b1 = (back >> 8) & 7u, b2 = (back >> 11) & 7u;
                s = s == b1 ? b2 : b1;
            }
        }
        bp[s0] = (uint16_t)s;
        count += s != z;
    }
    __syncthreads();

    // rule 5, both planes
    const int iz = (int)z;
    cs_write_plane(states + row * (int64_t)W, bp, W, lane, [iz](uint16_t v) { return (int)v - iz; });
    cs_write_plane(sign + row * (int64_t)W, bp, W, lane, [iz](uint16_t v) { return ((int)v > iz) - ((int)v < iz); });

    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
    if (lane == 0) nonneutral[row] = count;
}

}  // namespace icv

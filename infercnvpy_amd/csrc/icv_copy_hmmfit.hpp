// tl.cnv_copy_states_fit: the E-step of the Baum-Welch fit of the K-state model of tl.cnv_copy_states,
// 2 <= K <= 8.  Forward-backward along every chromosome of every cell by the rules k_copy_posterior_chains runs
// (icv_copy_posterior.hpp), but the posteriors are reduced to 2K + 1 sums per cell instead of leaving as planes: the
// K-state sibling of k_posterior_stats (icv_hmmfit.hpp).  tests/_copy_fit_oracle.py restates the contract.
//
// Float64 throughout, every operation one correctly rounded IEEE operation in the written order (the library is built
// -ffp-contract=off).  Rules 1-6 of 4.23 give b, al_t, c_t, be_t, w, z_t and gamma_t unchanged.  Per chromosome of T >= 1
// windows 2K + 1 sums start at 0.0 and take their terms for t = T-1 down to 0:
//   N_s += gamma_t(s)                 s = 0 .. K-1: the expected number of windows in state s
//   M_s += gamma_t(s) x_t             the product rounded before the add: the first moment of their values
//   for t <= T-2, with g(s) = b_{t+1}(s) be_{t+1}(s) (rule 4's g), m(s) = (al_t(s) ps) g(s),
//   st = (..(m(0) + m(1)) + ..) + m(K-1):
//   S += (st / c_{t+1}) / z_t         the expected number of steps that stay in their state
// The cell's sums start at 0.0 and add the chromosome sums in ascending chromosome order; a chromosome without windows
// adds nothing, nor does a window that no chromosome covers.  stats[i] = (N_0 .. N_{K-1}, M_0 .. M_{K-1}, S).  With the
// means (-a, 0.0, a) every operation that forms S is the one k_posterior_stats performs, and so are the bytes of S.
//
// Geometry: that of k_copy_posterior_chains: one wavefront per cell, the row through hmm_load_row, lane c running the
// chromosomes c, c + 64, ..., K a template parameter with everything per state in registers.  The forward pass is the one
// of cp_forward_backward (al_t into K planes of W doubles); the backward pass is written out here, because it keeps
// gamma_t in registers and stores no plane.  One chain for both kernels was built twice and put back (DESIGN.md 4.24,
// "One chain, measured"): a per-step sink as hmm_forward_backward has one, and __forceinline__ helpers for the forward
// pass and the recurrence step.  Either changes the compiled code of all 56 instantiations (a helper for the forward pass
// alone does), and each left one kernel slower than the run-to-run spread of the code as it is.
// st / c_{t+1} is formed in the step that reads al_t from LDS, where g and c_{t+1} are live, and carried as one double to
// the next step, where z_t is known.
//
// LDS: the row (W doubles), the K planes (K W doubles) and a tail of (2K + 1) n_chr doubles, statistic k of chromosome c
// at tail[k n_chr + c].  (The three-state kernel parks a chromosome's sums in the planes' slots of its first window; a
// chromosome of one window has only K + 1 such slots for 2K + 1 sums.)  After a barrier the lanes 0 .. 2K each add one
// statistic along the chromosomes in ascending order.  (Per-lane partial sums reduced by shuffles would fix neither the
// order for more than 64 chromosomes nor a sequential shape.)  8 (K + 1) W + 8 (2K + 1) n_chr bytes per cell, within
// kCpLdsBytes.  The only store to memory is 8 (2K + 1) bytes per cell; there are no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_copy_posterior.hpp"  // CsParams, cp_emit, cp_pred, cp_sum, kCpLdsBytes
#include "icv_hmm.hpp"             // hmm_load_row, hmm_chr

namespace icv {

// = ICV_COPY_POSTERIOR_STATS_LDS(n_cols, k, n_chr)
inline int64_t cps_lds_bytes(int64_t n_windows, int k, int64_t n_chr) {
    return 8 * ((int64_t)(k + 1) * n_windows + (int64_t)(2 * k + 1) * n_chr);
}
// = ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(k, n_chr); 0 where the tail alone takes the budget
inline int cps_max_windows(int k, int64_t n_chr) {
    const int64_t tail = 8 * (int64_t)(2 * k + 1) * (n_chr < 0 ? 0 : n_chr);
    return tail >= kCpLdsBytes ? 0 : (int)((kCpLdsBytes - tail) / (8 * (k + 1)));
}

// The sums of the windows [s0, s1), s1 > s0, of one chromosome.  x: the row; g: K planes of W doubles, plane s at
// g + s W, where the forward pass leaves al_t.  N, M: K sums each, S: one.
template <int K>
__device__ __forceinline__ void cps_chain_stats(const double* x, double* g, int32_t W, int32_t s0, int32_t s1,
                                                const CsParams& P, double (&N)[K], double (&M)[K], double& S) {
    double b[K], a[K], p[K], u[K];
    // rule 3, as cp_forward_backward runs it
    cp_emit<K>(x[s0], P, b);
    {
        const double cc = cp_sum<K>(b);
#pragma unroll
        for (int s = 0; s < K; ++s) a[s] = b[s] / cc, g[(size_t)s * W + s0] = a[s];
    }
    for (int32_t t = s0 + 1; t < s1; ++t) {
        cp_emit<K>(x[t], P, b);
        cp_pred<K>(a, P, p);
#pragma unroll
        for (int s = 0; s < K; ++s) u[s] = p[s] * b[s];
        const double cc = cp_sum<K>(u);
#pragma unroll
        for (int s = 0; s < K; ++s) a[s] = u[s] / cc, g[(size_t)s * W + t] = a[s];
    }
    // rules 4-5 and the sums: a = al_t
    double be[K];
#pragma unroll
    for (int s = 0; s < K; ++s) be[s] = 1.0, N[s] = 0.0, M[s] = 0.0;
    S = 0.0;
    double stay = 0.0;  // st / c_{t+1} of the window t in hand; there is none at t = T - 1
    for (int32_t t = s1 - 1;; --t) {
        const double xt = x[t];
        double w[K];
#pragma unroll
        for (int s = 0; s < K; ++s) w[s] = a[s] * be[s];
        const double z = cp_sum<K>(w);
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const double ga = w[s] / z;
            N[s] += ga;
            M[s] += ga * xt;
        }
        if (t != s1 - 1) S += stay / z;
        if (t == s0) break;
        cp_emit<K>(xt, P, b);  // b_t: the window the step t - 1 looks ahead to
#pragma unroll
        for (int s = 0; s < K; ++s) a[s] = g[(size_t)s * W + (t - 1)];
        cp_pred<K>(a, P, p);
#pragma unroll
        for (int s = 0; s < K; ++s) u[s] = p[s] * b[s];
        const double cc = cp_sum<K>(u);  // c_t, as the forward pass formed it
        double q[K], m[K];
#pragma unroll
        for (int s = 0; s < K; ++s) q[s] = b[s] * be[s];
#pragma unroll
        for (int s = 0; s < K; ++s) m[s] = (a[s] * P.stay) * q[s];  // a = al_{t-1}, q = rule 4's g at t
        stay = cp_sum<K>(m) / cc;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            double acc = (r == 0 ? P.stay : P.sw) * q[0];
#pragma unroll
            for (int s = 1; s < K; ++s) acc = acc + ((r == s ? P.stay : P.sw) * q[s]);
            be[r] = acc / cc;
        }
    }
}

// chr_start: see hmm_chr.  stats: n x (2K + 1).  Dynamic LDS: cps_lds_bytes(W, K, C).
template <typename T, bool CSR, int K>
__global__ __launch_bounds__(64) void k_copy_posterior_stats(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                             const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                             const int32_t* __restrict__ chr_start, int32_t C, CsParams P,
                                                             double* __restrict__ stats) {
    static_assert(K >= 2 && K <= kCsMaxStates, "the model of icv_copy_states_viterbi");
    static_assert(2 * K + 1 <= 64, "one lane per statistic");
    extern __shared__ __attribute__((aligned(16))) unsigned char cps_lds[];
    double* x = reinterpret_cast<double*>(cps_lds);
    double* g = x + W;                    // plane s at g + s W: al_t(s)
    double* tail = g + (size_t)K * W;     // statistic k of chromosome c at tail[k C + c]
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;

    hmm_load_row<T, CSR>(x, W, val, indptr, indices, ld, row, lane);

    for (int32_t c = lane; c < C; c += 64) {
        int32_t s0, s1;
        if (!hmm_chr(chr_start, c, W, s0, s1)) continue;
        double N[K], M[K], S;
        cps_chain_stats<K>(x, g, W, s0, s1, P, N, M, S);
#pragma unroll
        for (int s = 0; s < K; ++s) tail[(size_t)s * C + c] = N[s], tail[(size_t)(K + s) * C + c] = M[s];
        tail[(size_t)(2 * K) * C + c] = S;
    }
    __syncthreads();

    // lane k adds statistic k of the chromosomes in ascending order
    if (lane < 2 * K + 1) {
        const double* mine = tail + (size_t)lane * C;
        double acc = 0.0;
        for (int32_t c = 0; c < C; ++c) {
            int32_t s0, s1;
            if (hmm_chr(chr_start, c, W, s0, s1)) acc += mine[c];
        }
        stats[row * (2 * K + 1) + lane] = acc;
    }
}

}  // namespace icv

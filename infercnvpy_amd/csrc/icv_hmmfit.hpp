// tl.cnv_states_fit: the E-step of the Baum-Welch fit of amplitude, sigma and switch_prob of the
// three-state model of tl.cnv_states.  Forward-backward along every chromosome of every cell by the chain that
// k_posterior_chains runs (hmm_forward_backward of icv_hmm.hpp), but the posteriors are reduced to three sums per cell
// instead of leaving as n x W planes.  tests/_fit_oracle.py restates the contract.
//
// Float64 throughout, every operation one correctly rounded IEEE operation in the written order (the library is built
// -ffp-contract=off).  Rules 1-5 of 4.15 give b, al_t, c_t, be_t, w, z_t and gamma_t unchanged.  Per chromosome of T
// windows three sums start at 0.0 and take their terms for t = T-1 down to 0:
//   G += (gamma_t(0) + gamma_t(2))                          the expected number of altered windows
//   D += (gamma_t(2) - gamma_t(0)) x_t                      the signed first moment of their values
//   for t <= T-2, with g(s) = b_{t+1}(s) be_{t+1}(s) (rule 4's g), m(s) = (al_t(s) ps) g(s), st = (m(0) + m(1)) + m(2):
//   K += (st / c_{t+1}) / z_t                               the expected number of steps that stay in their state
// The cell's G, D and K start at 0.0 and add the chromosome sums in ascending chromosome order; a chromosome without
// windows adds nothing.  stats[i] = (G, D, K).
//
// Geometry: that of icv_hmm.hpp and k_posterior_chains: the row as W doubles and al_t as three planes of W doubles in
// LDS (32 bytes per window).
// The backward pass keeps gamma_t in registers.  When a chromosome's chain is finished nothing reads the planes' slots of
// its first window again: its three sums are parked there, and after a barrier three lanes, one per statistic, add them
// up along chr_start.  (Per-lane partial sums reduced by shuffles would fix neither the order for more than 64
// chromosomes nor a sequential shape.)  The only store to memory is 24 bytes per cell; there are no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_hmm.hpp"        // PoParams, hmm_load_row, hmm_chr, hmm_forward_backward
#include "icv_posterior.hpp"  // po_lds_bytes, kPoMaxWindows

namespace icv {

// chr_start: see hmm_chr.  stats: n x 3.
template <typename T, bool CSR>
__global__ __launch_bounds__(64) void k_posterior_stats(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                        const int32_t* __restrict__ chr_start, int32_t C, PoParams P,
                                                        double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hf_lds[];
    double* x = reinterpret_cast<double*>(hf_lds);
    double* g0 = x + W;  // al_t(0); at a chromosome's first window, once its chain is done, its G
    double* g1 = x + 2 * (size_t)W;  // al_t(1); its D
    double* g2 = x + 3 * (size_t)W;  // al_t(2); its K
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;

    hmm_load_row<T, CSR>(x, W, val, indptr, indices, ld, row, lane);

    for (int32_t c = lane; c < C; c += 64) {
        int32_t s0, s1;
        if (!hmm_chr(chr_start, c, W, s0, s1)) continue;
        double G = 0.0, D = 0.0, K = 0.0;
        hmm_forward_backward(x, g0, g1, g2, s0, s1, P, [&](const HmmStep& s) {
            const double ga0 = s.w0 / s.z, ga2 = s.w2 / s.z;
            G += (ga0 + ga2);
            D += (ga2 - ga0) * x[s.t];
            if (s.inner) {
                const double m0 = (s.a0 * P.ps) * s.q0, m1 = (s.a1 * P.ps) * s.q1, m2 = (s.a2 * P.ps) * s.q2;
                const double st = (m0 + m1) + m2;
                K += (st / s.cc) / s.z;
            }
        });
        g0[s0] = G, g1[s0] = D, g2[s0] = K;
    }
    __syncthreads();

    // lane k adds statistic k of the chromosomes in ascending order
    if (lane < 3) {
        const double* plane = x + (size_t)(lane + 1) * W;
        double acc = 0.0;
        for (int32_t c = 0; c < C; ++c) {
            int32_t s0, s1;
            if (hmm_chr(chr_start, c, W, s0, s1)) acc += plane[s0];
        }
        stats[row * 3 + lane] = acc;
    }
}

}  // namespace icv

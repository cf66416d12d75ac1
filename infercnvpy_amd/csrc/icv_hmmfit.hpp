// tl.cnv_states_fit: the E-step of the Baum-Welch fit of amplitude, sigma and switch_prob of the
// three-state model of tl.cnv_states.  Forward-backward along every chromosome of every cell as in k_posterior_chains,
// but the posteriors are reduced to three sums per cell instead of leaving as n x W planes.  tests/_fit_oracle.py
// restates the contract.
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
// Geometry: that of k_posterior_chains, one wavefront (a 64-thread workgroup) per cell, lane c running the chromosomes
// c, c + 64, ... sequentially, the row as W doubles and al_t as three planes of W doubles in LDS (32 bytes per window).
// The backward pass keeps gamma_t in registers.  When a chromosome's chain is finished nothing reads the planes' slots of
// its first window again: its three sums are parked there, and after a barrier three lanes, one per statistic, add them
// up along chr_start.  (Per-lane partial sums reduced by shuffles would fix neither the order for more than 64
// chromosomes nor a sequential shape.)  The only store to memory is 24 bytes per cell; there are no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_posterior.hpp"  // PoParams, po_emit, po_pred, po_lds_bytes, kPoMaxWindows

namespace icv {

// chr_start: C + 1 ascending window numbers, chr_start[0] = 0, chr_start[C] = W (the host checked them; they are clamped
// to [0, W] here all the same, so no LDS access leaves the row).  stats: n x 3.
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

    if (CSR) {
        for (int32_t j = lane; j < W; j += 64) x[j] = 0.0;
        __syncthreads();
        const int64_t b = indptr[row], e = indptr[row + 1];
        for (int64_t k = b + lane; k < e; k += 64) {
            const int32_t c = indices[k];
            if ((uint32_t)c < (uint32_t)W) x[c] = (double)val[k];
        }
    } else {
        const T* src = val + row * ld;
        for (int32_t j = lane; j < W; j += 64) x[j] = (double)src[j];
    }
    __syncthreads();

    for (int32_t c = lane; c < C; c += 64) {
        const int32_t s0 = min(max(chr_start[c], 0), W), s1 = min(max(chr_start[c + 1], 0), W);
        if (s1 <= s0) continue;
        double b0, b1, b2, a0, a1, a2;
        // rule 3 of 4.15
        po_emit(x[s0], P, b0, b1, b2);
        {
            const double cc = (b0 + b1) + b2;
            a0 = b0 / cc, a1 = b1 / cc, a2 = b2 / cc;
        }
        g0[s0] = a0, g1[s0] = a1, g2[s0] = a2;
        for (int32_t t = s0 + 1; t < s1; ++t) {
            double p0, p1, p2;
            po_emit(x[t], P, b0, b1, b2);
            po_pred(a0, a1, a2, P, p0, p1, p2);
            const double u0 = p0 * b0, u1 = p1 * b1, u2 = p2 * b2;
            const double cc = (u0 + u1) + u2;
            a0 = u0 / cc, a1 = u1 / cc, a2 = u2 / cc;
            g0[t] = a0, g1[t] = a1, g2[t] = a2;
        }
        // rules 4-5 and the sums: (a0, a1, a2) = al_t; from the second step on (q0, q1, q2) = b_{t+1} be_{t+1} and
        // cc = c_{t+1}
        double be0 = 1.0, be1 = 1.0, be2 = 1.0;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, cc = 1.0;
        double G = 0.0, D = 0.0, K = 0.0;
        for (int32_t t = s1 - 1;; --t) {
            const double w0 = a0 * be0, w1 = a1 * be1, w2 = a2 * be2;
            const double z = (w0 + w1) + w2;
            const double ga0 = w0 / z, ga2 = w2 / z;
            G += (ga0 + ga2);
            D += (ga2 - ga0) * x[t];
            if (t != s1 - 1) {
                const double m0 = (a0 * P.ps) * q0, m1 = (a1 * P.ps) * q1, m2 = (a2 * P.ps) * q2;
                const double st = (m0 + m1) + m2;
                K += (st / cc) / z;
            }
            if (t == s0) break;
            po_emit(x[t], P, b0, b1, b2);  // b_t: the window the step t - 1 looks ahead to
            a0 = g0[t - 1], a1 = g1[t - 1], a2 = g2[t - 1];
            double p0, p1, p2;
            po_pred(a0, a1, a2, P, p0, p1, p2);
            cc = ((p0 * b0) + (p1 * b1)) + (p2 * b2);  // c_t, as the forward pass formed it
            q0 = b0 * be0, q1 = b1 * be1, q2 = b2 * be2;
            const double v0 = ((P.ps * q0) + (P.pw * q1)) + (P.pw * q2);
            const double v1 = ((P.pw * q0) + (P.ps * q1)) + (P.pw * q2);
            const double v2 = ((P.pw * q0) + (P.pw * q1)) + (P.ps * q2);
            be0 = v0 / cc, be1 = v1 / cc, be2 = v2 / cc;
        }
        g0[s0] = G, g1[s0] = D, g2[s0] = K;
    }
    __syncthreads();

    // lane k adds statistic k of the chromosomes in ascending order
    if (lane < 3) {
        const double* plane = x + (size_t)(lane + 1) * W;
        double acc = 0.0;
        for (int32_t c = 0; c < C; ++c) {
            const int32_t s0 = min(max(chr_start[c], 0), W), s1 = min(max(chr_start[c + 1], 0), W);
            if (s1 <= s0) continue;
            acc += plane[s0];
        }
        stats[row * 3 + lane] = acc;
    }
}

}  // namespace icv

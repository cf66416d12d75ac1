// What k_states_viterbi, k_posterior_chains, k_posterior_stats and k_copy_states_viterbi share (DESIGN.md 4.13, 4.15, 4.16,
// 4.22).
// Geometry: one wavefront (a 64-thread workgroup) per cell.  The row lies in LDS as W doubles (zeroed, then the stored
// entries scattered on top; a dense row is converted in place), lane c runs the chromosomes c, c + 64, ... sequentially.
// The forward-backward chain of 4.15 is written here once: 4.16 needs b, al_t, c_t, be_t, w and z bit for bit as 4.15
// forms them, so both kernels run this one function and differ only in the sink that takes (w, z) at each window.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_tsne.hpp"  // ts_exp

namespace icv {

// the row of one cell into x[0, W); ends with a barrier.  (The kernels' parameters carry __restrict__; repeated here it
// gave k_states_viterbi another schedule, measured 0.4 % slower.)
template <typename T, bool CSR>
__device__ __forceinline__ void hmm_load_row(double* x, int32_t W, const T* val, const int64_t* indptr,
                                             const int32_t* indices, int64_t ld, int64_t row, int lane) {
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
}

// the windows [s0, s1) of chromosome c; false when it has none.  chr_start: C + 1 ascending window numbers,
// chr_start[0] = 0, chr_start[C] = W (the host checked them; they are clamped to [0, W] here all the same, so no LDS
// access leaves the row).
__device__ __forceinline__ bool hmm_chr(const int32_t* __restrict__ chr_start, int32_t c, int32_t W, int32_t& s0,
                                        int32_t& s1) {
    s0 = min(max(chr_start[c], 0), W), s1 = min(max(chr_start[c + 1], 0), W);
    return s1 > s0;
}

struct PoParams {
    double a, h, ps, pw;
};

// rule 2 of 4.15 for the three states
__device__ __forceinline__ void po_emit(double x, const PoParams& P, double& b0, double& b1, double& b2) {
    const double t0 = x - (-P.a), t1 = x - 0.0, t2 = x - P.a;
    const double e0 = -(t0 * t0) * P.h, e1 = -(t1 * t1) * P.h, e2 = -(t2 * t2) * P.h;
    double m = e0;
    if (e1 > m) m = e1;
    if (e2 > m) m = e2;
    b0 = ts_exp(e0 - m);
    b1 = ts_exp(e1 - m);
    b2 = ts_exp(e2 - m);
}

// pred of rule 3 from al_{t-1}
__device__ __forceinline__ void po_pred(double a0, double a1, double a2, const PoParams& P, double& p0, double& p1,
                                        double& p2) {
    p0 = ((a0 * P.ps) + (a1 * P.pw)) + (a2 * P.pw);
    p1 = ((a0 * P.pw) + (a1 * P.ps)) + (a2 * P.pw);
    p2 = ((a0 * P.pw) + (a1 * P.pw)) + (a2 * P.ps);
}

// window t of the backward pass, as the sink gets it
struct HmmStep {
    int32_t t;
    bool inner;             // t < T - 1: q and cc exist
    double a0, a1, a2;      // al_t
    double w0, w1, w2, z;   // rule 5
    double q0, q1, q2, cc;  // b_{t+1} be_{t+1} (rule 4's g) and c_{t+1}
};

// Rules 3-5 of 4.15 over the windows [s0, s1), s1 > s0, of one chromosome.  x: the row; g0, g1, g2: three planes of W
// doubles, where the forward pass leaves al_t.  The backward pass calls sink(HmmStep) for t = s1 - 1 down to s0; the
// sink may overwrite the planes at t: al_{t-1} is read after it returns.
template <typename Sink>
__device__ __forceinline__ void hmm_forward_backward(const double* x, double* g0, double* g1, double* g2, int32_t s0,
                                                     int32_t s1, const PoParams& P, Sink&& sink) {
    double b0, b1, b2, a0, a1, a2;
    // rule 3
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
    // rules 4-5: (a0, a1, a2) = al_t
    double be0 = 1.0, be1 = 1.0, be2 = 1.0;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, cc = 1.0;
    for (int32_t t = s1 - 1;; --t) {
        const double w0 = a0 * be0, w1 = a1 * be1, w2 = a2 * be2;
        const double z = (w0 + w1) + w2;
        sink(HmmStep{t, t != s1 - 1, a0, a1, a2, w0, w1, w2, z, q0, q1, q2, cc});
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
}

}  // namespace icv

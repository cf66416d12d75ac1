// tl.cnv_copy_posteriors and tl.cnv_copy_states_filter: the posterior probabilities of the K-state model of
// tl.cnv_copy_states, 2 <= K <= 8, by forward-backward along every chromosome, and the filter that resets to neutral every
// called run of one level whose mean P(neutral) exceeds a threshold.  tests/_copy_posterior_oracle.py restates both
// contracts.
//
// Posteriors: the K-state form of 4.15, float64 throughout, every operation one correctly rounded IEEE operation in the
// written order (the library is built -ffp-contract=off):
//   1. host scalars, passed as doubles: h = 1.0 / (2.0 sigma sigma), ps = 1.0 - p, pw = p / (K - 1) (a normal float64);
//      A(r, s) = ps for r = s and pw otherwise; the state means mu_0 < ... < mu_{K-1} with mu_z = 0.0 are passed by value.
//   2. emissions: t = x - mu_s, e_s = -(t t) h; m = e_0, then for s = 1 .. K-1: if e_s > m then m = e_s;
//      b(s) = exp_(e_s - m) with the written exponential ts_exp of icv_tsne.hpp.
//   3. forward: u_0(s) = b_0(s); for t >= 1 pred(s) = (..((al(0) A(0,s)) + (al(1) A(1,s))) + ..) + (al(K-1) A(K-1,s)) over
//      al_{t-1}, r ascending, and u_t(s) = pred(s) b_t(s); c_t = (..(u(0) + u(1)) + ..) + u(K-1), al_t(s) = u_t(s) / c_t.
//   4. backward: be_{T-1}(s) = 1.0; g(s) = b_{t+1}(s) be_{t+1}(s), v(r) = (..((A(r,0) g(0)) + (A(r,1) g(1))) + ..), s
//      ascending, be_t(r) = v(r) / c_{t+1}.
//   5. w(s) = al_t(s) be_t(s), z = (..(w(0) + w(1)) + ..), gamma_t(s) = w(s) / z.
//   6. chains never cross a chromosome boundary; an entry that is not stored is 0.0; a window that no chromosome covers
//      has gamma = 1.0 for the neutral state and 0.0 elsewhere.
// The K^2 sums of rules 3 and 4 are the contract: al(s) ps + (S - al(s)) pw rounds differently.  With the means
// (-a, 0.0, a) every operation is the one hmm_forward_backward of icv_hmm.hpp performs, and so are the bytes.
//
// Geometry: that of icv_hmm.hpp (one wavefront per cell, the row through hmm_load_row, lane c running the chromosomes
// c, c + 64, ...).  K is a template parameter: al, b, be, g stay in registers, every loop over the states is unrolled and
// no array is indexed by a run-time value; the means are kernel arguments.  LDS holds the row as W doubles and K planes of
// W doubles: the forward pass leaves al_t there, the backward pass reads al_{t-1}, recomputes b_t and c_t (the same
// operations on the same operands, hence the same bits) and overwrites al_t with gamma_t; the planes then leave in
// coalesced 8-byte stores.  8 (K + 1) bytes of LDS per window and resident cell.
//
// Filter: the rules of 4.15's filter on calls that are levels in [-7, 7]:
//   1. q_t = int64(rint(P[i,t] 2^40)).
//   2. a run [s, e) is a maximal stretch of ONE level other than 0 inside one chromosome (+1 +1 +2 +2 is two runs); it has
//      S = the int64 sum of its q_t and mean = double(S) / (double(e - s) 2^40).
//   3. the run is reset to 0 iff mean > max_p_normal.
// Geometry and body: those of k_states_filter; both kernels run fi_filter_row (icv_posterior.hpp), here with the wider
// range and the second output plane.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_copy_states.hpp"  // CsParams, kCsMaxStates
#include "icv_posterior.hpp"    // kFiRowsPerBlock, fi_filter_row

namespace icv {

constexpr int kCpLdsBytes = 163840;  // = ICV_COPY_POSTERIOR_LDS_BYTES: the CU's 160 KiB
constexpr int cp_max_windows(int k) { return kCpLdsBytes / (8 * (k + 1)); }  // = ICV_COPY_POSTERIOR_MAX_WINDOWS(k)
constexpr int kCfMaxLevel = 7;       // a call of icv_copy_states_viterbi lies in [-7, 7]

inline size_t cp_lds_bytes(int32_t n_windows, int k) { return (size_t)n_windows * 8 * (size_t)(k + 1); }

// rule 2 for the K states
template <int K>
__device__ __forceinline__ void cp_emit(double x, const CsParams& P, double (&b)[K]) {
    double e[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const double t = x - P.mu[s];
        e[s] = -(t * t) * P.h;
    }
    double m = e[0];
#pragma unroll
    for (int s = 1; s < K; ++s)
        if (e[s] > m) m = e[s];
#pragma unroll
    for (int s = 0; s < K; ++s) b[s] = ts_exp(e[s] - m);
}

// pred of rule 3 from al_{t-1}; P.stay, P.sw: ps, pw of rule 1
template <int K>
__device__ __forceinline__ void cp_pred(const double (&a)[K], const CsParams& P, double (&p)[K]) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
        double acc = a[0] * (s == 0 ? P.stay : P.sw);
#pragma unroll
        for (int r = 1; r < K; ++r) acc = acc + (a[r] * (r == s ? P.stay : P.sw));
        p[s] = acc;
    }
}

// (..(v(0) + v(1)) + ..) + v(K-1)
template <int K>
__device__ __forceinline__ double cp_sum(const double (&v)[K]) {
    double acc = v[0];
#pragma unroll
    for (int s = 1; s < K; ++s) acc = acc + v[s];
    return acc;
}

// Rules 3-5 over the windows [s0, s1), s1 > s0, of one chromosome: the K-state sibling of hmm_forward_backward.  x: the
// row; g: K planes of W doubles, plane s at g + s W, where the forward pass leaves al_t and the backward pass gamma_t.
template <int K>
__device__ __forceinline__ void cp_forward_backward(const double* x, double* g, int32_t W, int32_t s0, int32_t s1,
                                                    const CsParams& P) {
    double b[K], a[K], p[K], u[K];
    // rule 3
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
    // rules 4-5: a = al_t
    double be[K];
#pragma unroll
    for (int s = 0; s < K; ++s) be[s] = 1.0;
    for (int32_t t = s1 - 1;; --t) {
        double w[K];
#pragma unroll
        for (int s = 0; s < K; ++s) w[s] = a[s] * be[s];
        const double z = cp_sum<K>(w);
#pragma unroll
        for (int s = 0; s < K; ++s) g[(size_t)s * W + t] = w[s] / z;
        if (t == s0) break;
        cp_emit<K>(x[t], P, b);  // b_t: the window the step t - 1 looks ahead to
#pragma unroll
        for (int s = 0; s < K; ++s) a[s] = g[(size_t)s * W + (t - 1)];
        cp_pred<K>(a, P, p);
#pragma unroll
        for (int s = 0; s < K; ++s) u[s] = p[s] * b[s];
        const double cc = cp_sum<K>(u);  // c_t, as the forward pass formed it
        double q[K];
#pragma unroll
        for (int s = 0; s < K; ++s) q[s] = b[s] * be[s];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            double acc = (r == 0 ? P.stay : P.sw) * q[0];
#pragma unroll
            for (int s = 1; s < K; ++s) acc = acc + ((r == s ? P.stay : P.sw) * q[s]);
            be[r] = acc / cc;
        }
    }
}

// chr_start: see hmm_chr.  neutral: n x W; planes: K x n x W (plane s = P(state s)) or null.
template <typename T, bool CSR, int K>
__global__ __launch_bounds__(64) void k_copy_posterior_chains(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                              const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                              const int32_t* __restrict__ chr_start, int32_t C, CsParams P,
                                                              double* __restrict__ neutral, double* __restrict__ planes) {
    static_assert(K >= 2 && K <= kCsMaxStates, "the model of icv_copy_states_viterbi");
    extern __shared__ __attribute__((aligned(16))) unsigned char cp_lds[];
    double* x = reinterpret_cast<double*>(cp_lds);
    double* g = x + W;  // plane s at g + s W: al_t(s), then gamma_t(s)
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int z = min(max(P.z, 0), K - 1);  // (the host checked it; no LDS access leaves the planes)

    // (a window no chromosome covers is neutral)
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const double v = s == z ? 1.0 : 0.0;
        for (int32_t j = lane; j < W; j += 64) g[(size_t)s * W + j] = v;
    }
    hmm_load_row<T, CSR>(x, W, val, indptr, indices, ld, row, lane);

    for (int32_t c = lane; c < C; c += 64) {
        int32_t s0, s1;
        if (!hmm_chr(chr_start, c, W, s0, s1)) continue;
        cp_forward_backward<K>(x, g, W, s0, s1, P);
    }
    __syncthreads();

    double* out = neutral + row * (int64_t)W;
    const double* gz = g + (size_t)z * W;
    for (int32_t j = lane; j < W; j += 64) out[j] = gz[j];
    if (planes != nullptr) {
        const int64_t plane = (int64_t)gridDim.x * W;  // n W
#pragma unroll
        for (int s = 0; s < K; ++s) {
            double* o = planes + s * plane + row * (int64_t)W;
            for (int32_t j = lane; j < W; j += 64) o[j] = g[(size_t)s * W + j];
        }
    }
}

// ---- the filter -------------------------------------------------------------------------------------------------------
// fi_filter_row (icv_posterior.hpp) on levels in [-7, 7], with the sign plane
__global__ __launch_bounds__(64 * kFiRowsPerBlock) void k_copy_states_filter(
    const int8_t* __restrict__ S, const double* __restrict__ Pn, int64_t n_rows, int32_t W,
    const uint32_t* __restrict__ mask, double thr, int8_t* __restrict__ out, int8_t* __restrict__ sign,
    int32_t* __restrict__ nonneutral, int32_t* __restrict__ removed, int32_t* __restrict__ bad) {
    const int64_t row = (int64_t)blockIdx.x * kFiRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (whole wavefronts leave; there is no barrier below)
    fi_filter_row<kCfMaxLevel, true>(S, Pn, row, W, mask, thr, out, sign, nonneutral, removed, bad);
}

}  // namespace icv

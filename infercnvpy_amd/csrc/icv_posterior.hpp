// tl.cnv_posteriors and tl.cnv_states_filter: the posterior probabilities of the three-state model of
// tl.cnv_states by forward-backward along every chromosome, and the filter that resets to neutral every called segment
// whose mean P(neutral) exceeds a threshold (R inferCNV's BayesMaxPNormal).  tests/_posterior_oracle.py restates both
// contracts.
//
// Posteriors, float64 throughout, every operation one correctly rounded IEEE operation in the written order (the
// library is built -ffp-contract=off):
//   1. host scalars, passed as doubles: h = 1.0 / (2.0 sigma sigma), ps = 1.0 - p, pw = p / 2.0 (a normal float64);
//      A(r, s) = ps for r = s and pw otherwise.
//   2. emissions: t = x - mu_s, e_s = -(t t) h (rule 2 of 4.13); m = max(e_0, e_1, e_2); b(s) = exp_(e_s - m) with the
//      written exponential ts_exp of icv_tsne.hpp.  The largest b is exactly 1.0.
//   3. forward: u_0(s) = b_0(s); for t >= 1 pred(s) = ((al(0) A(0,s)) + (al(1) A(1,s))) + (al(2) A(2,s)) over al_{t-1}
//      and u_t(s) = pred(s) b_t(s); c_t = (u(0) + u(1)) + u(2), al_t(s) = u_t(s) / c_t.
//   4. backward: be_{T-1}(s) = 1.0; g(s) = b_{t+1}(s) be_{t+1}(s), v(r) = ((A(r,0) g(0)) + (A(r,1) g(1))) + (A(r,2) g(2)),
//      be_t(r) = v(r) / c_{t+1}.
//   5. w(s) = al_t(s) be_t(s), z = (w(0) + w(1)) + w(2), gamma_t(s) = w(s) / z.
//   6. chains never cross a chromosome boundary; an entry that is not stored is 0.0.
//
// Geometry: that of icv_hmm.hpp, which also holds the chain (hmm_forward_backward).  LDS holds the row as W doubles and
// three planes of W doubles: the forward pass leaves al_t there, the backward pass reads al_t, recomputes b_{t+1} and
// c_{t+1} (the same operations on the same operands, hence the same bits) and overwrites al_t with gamma_t; the planes
// then leave in coalesced 8-byte stores.  32 bytes of LDS per window and resident cell.
//
// Filter, integers after one rounding per window:
//   1. q_t = int64(rint(P[i,t] 2^40)).
//   2. a run [s, e) (rule 1 of 4.14) has S = the int64 sum of its q_t and mean = double(S) / (double(e - s) 2^40).
//   3. the run is reset to 0 iff mean > max_p_normal.
// Geometry: one wavefront per row, four rows per workgroup, one window per lane and step of 64 windows.  A wavefront
// prefix sum of q plus the ballots of the run starts and ends give every run's sum at its last window; the carry of a
// run that is open at the end of a step is one (start, sum) pair.  A window of a run is written when the run's end has
// been seen: by its own lane if that is in the same step, by the whole wavefront otherwise.  Every output byte is
// written exactly once; no row is held in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_hmm.hpp"       // PoParams, hmm_load_row, hmm_chr, hmm_forward_backward
#include "icv_segments.hpp"  // kSegMaskShift, k_seg_chr_mask

namespace icv {

constexpr int kPoMaxWindows = 4096;  // = ICV_POSTERIOR_MAX_WINDOWS: 32 x 4096 = 128 KiB of the CU's 160 KiB
constexpr int kPoLdsPerWindow = 32;  // the float64 value + three float64 planes
constexpr int kFiRowsPerBlock = 4;   // wavefronts (rows) per workgroup of k_states_filter
constexpr int kFiMaxWindows = 1 << 22;  // 2^22 terms of at most 2^40 fit an int64

inline size_t po_lds_bytes(int32_t n_windows) { return (size_t)n_windows * kPoLdsPerWindow; }

// chr_start: see hmm_chr.  neutral: n x W; loss / gain: n x W or both null.
template <typename T, bool CSR>
__global__ __launch_bounds__(64) void k_posterior_chains(const T* __restrict__ val, const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices, int64_t ld, int32_t W,
                                                         const int32_t* __restrict__ chr_start, int32_t C, PoParams P,
                                                         double* __restrict__ neutral, double* __restrict__ loss,
                                                         double* __restrict__ gain) {
    extern __shared__ __attribute__((aligned(16))) unsigned char po_lds[];
    double* x = reinterpret_cast<double*>(po_lds);
    double* g0 = x + W;       // al_t(0), then gamma_t(0)
    double* g1 = x + 2 * (size_t)W;
    double* g2 = x + 3 * (size_t)W;
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;

    // (a window no chromosome covers is neutral)
    for (int32_t j = lane; j < W; j += 64) g0[j] = 0.0, g1[j] = 1.0, g2[j] = 0.0;
    hmm_load_row<T, CSR>(x, W, val, indptr, indices, ld, row, lane);

    for (int32_t c = lane; c < C; c += 64) {
        int32_t s0, s1;
        if (!hmm_chr(chr_start, c, W, s0, s1)) continue;
        hmm_forward_backward(x, g0, g1, g2, s0, s1, P, [&](const HmmStep& s) {  // gamma_t (rule 5) over al_t
            g0[s.t] = s.w0 / s.z, g1[s.t] = s.w1 / s.z, g2[s.t] = s.w2 / s.z;
        });
    }
    __syncthreads();

    double* out = neutral + row * (int64_t)W;
    for (int32_t j = lane; j < W; j += 64) out[j] = g1[j];
    if (loss != nullptr && gain != nullptr) {
        double* ol = loss + row * (int64_t)W;
        double* og = gain + row * (int64_t)W;
        for (int32_t j = lane; j < W; j += 64) ol[j] = g0[j], og[j] = g2[j];
    }
}

// ---- the filter -------------------------------------------------------------------------------------------------------
// One row of the filter, for k_states_filter and k_copy_states_filter (icv_copy_posterior.hpp, rules of 4.23): calls in
// [-MaxLevel, MaxLevel], a run being a maximal stretch of ONE level other than 0 inside one chromosome (with MaxLevel = 1
// that is rule 1 of 4.14); Sign: the plane `sign` (out clipped to -1 / 0 / +1) is written too, otherwise it is not
// touched.  S, P, out, sign: n_rows x W row-major without padding; mask: the chromosome-start bits of k_seg_chr_mask (bit
// kSegMaskShift + t is window t; seg_mask_words(W) words).  nonneutral[row] = the windows of out's row that are not 0,
// removed[row] = the runs that were reset.  *bad |= 1 where a call is outside the range or a posterior is not a number
// in [0, 1] (such a posterior counts as 0).  W <= kFiMaxWindows.  Called by all 64 lanes of a wavefront; no barrier.
template <int MaxLevel, bool Sign>
__device__ __forceinline__ void fi_filter_row(const int8_t* __restrict__ S, const double* __restrict__ Pn, int64_t row,
                                              int32_t W, const uint32_t* __restrict__ mask, double thr,
                                              int8_t* __restrict__ out, int8_t* __restrict__ sign,
                                              int32_t* __restrict__ nonneutral, int32_t* __restrict__ removed,
                                              int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int8_t* s_row = S + row * (int64_t)W;
    const double* p_row = Pn + row * (int64_t)W;
    int8_t* o_row = out + row * (int64_t)W;
    int8_t* g_row = Sign ? sign + row * (int64_t)W : nullptr;
    auto put = [&](int32_t t, int v) {  // window t of out (and of sign)
        o_row[t] = (int8_t)v;
        if constexpr (Sign) g_row[t] = (int8_t)((v > 0) - (v < 0));
    };

    int32_t carry_state = 0;   // the call of the window in front of this step
    int32_t open_start = 0;    // the first window of the run that was open at the end of the step before
    int64_t open_sum = 0;      // its sum so far
    int32_t kept = 0, gone = 0;
    bool invalid = false;

    for (int32_t v0 = 0; v0 < W; v0 += 64) {
        const int32_t t = v0 + lane;
        const bool in = t < W;
        const int s = in ? (int)s_row[t] : 0;
        const double pv = in ? p_row[t] : 0.0;
        const bool p_ok = pv >= 0.0 && pv <= 1.0;  // (false for NaN)
        invalid |= s < -MaxLevel || s > MaxLevel || !p_ok;
        int prev = __shfl_up(s, 1, 64);
        if (lane == 0) prev = carry_state;
        int next = __shfl_down(s, 1, 64);
        if (lane == 63) next = (t + 1 < W) ? (int)s_row[t + 1] : 0;
        carry_state = __shfl(s, 63, 64);

        // is window t / t + 1 a chromosome start?  (bit kSegMaskShift + W is never set; the mask has the word)
        const uint32_t qb = (uint32_t)(in ? t : 0) + kSegMaskShift;
        const bool cs0 = (mask[qb >> 5] >> (qb & 31)) & 1u;
        const bool cs1 = (mask[(qb + 1) >> 5] >> ((qb + 1) & 31)) & 1u;
        const bool sf = s != 0 && (cs0 || prev != s);  // (another level starts another run)
        const bool ef = s != 0 && (cs1 || next != s);  // (t + 1 == W: next = 0)

        const int64_t q = (s != 0 && p_ok) ? (int64_t)rint(pv * 1099511627776.0) : 0;
        int64_t incl = q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const int64_t excl = incl - q;
        const uint64_t smask = __ballot(sf), emask = __ballot(ef);

        // the lane of this window's run start (-1: the run was open when the step began) and of its end (64: it stays open)
        const uint64_t below = smask & (~0ull >> (63 - lane));
        const int sl = below ? 63 - __builtin_clzll(below) : -1;
        const uint64_t above = emask >> lane;
        const int el = above ? lane + __builtin_ctzll(above) : 64;
        const int64_t excl_at_start = __shfl(excl, sl < 0 ? 0 : sl, 64);

        // the verdict, formed at the run's last window
        bool reset = false;
        if (ef) {
            const int64_t sum = sl >= 0 ? incl - excl_at_start : open_sum + incl;
            const int32_t first = sl >= 0 ? v0 + sl : open_start;
            const int32_t len = t + 1 - first;
            const double mean = (double)sum / ((double)len * 1099511627776.0);
            reset = mean > thr;
            if (reset) ++gone;
            else kept += len;
        }
        const bool my_reset = __shfl((int)reset, el & 63, 64) != 0;
        if (in) {
            if (s == 0) put(t, 0);
            else if (el < 64) put(t, my_reset ? 0 : s);
        }
        // the windows of the steps before that belong to a run ending in this step (the run of lane 0, if it was open)
        const int s_first = __shfl(s, 0, 64);
        const bool first_open = __shfl((int)(sl < 0 && s != 0 && el < 64), 0, 64) != 0;
        if (first_open) {
            const int v = __shfl((int)my_reset, 0, 64) != 0 ? 0 : s_first;
            for (int32_t k = open_start + lane; k < v0; k += 64) put(k, v);
        }
        // the run that stays open: lane 63's, if it has not ended
        const bool stays = __shfl((int)(s != 0 && el == 64), 63, 64) != 0;
        if (stays) {
            const int sl63 = __shfl(sl, 63, 64);
            const int64_t total = __shfl(incl, 63, 64);
            if (sl63 >= 0) {
                open_start = v0 + sl63;
                open_sum = total - __shfl(excl, sl63, 64);
            } else {
                open_sum += total;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        kept += __shfl_down(kept, off, 64);
        gone += __shfl_down(gone, off, 64);
    }
    if (lane == 0) nonneutral[row] = kept, removed[row] = gone;
    if (__ballot(invalid) != 0 && lane == 0) atomicOr(bad, 1);
}

// the calls -1 / 0 / +1 of tl.cnv_states: one wavefront per row, kFiRowsPerBlock rows per workgroup
__global__ __launch_bounds__(64 * kFiRowsPerBlock) void k_states_filter(
    const int8_t* __restrict__ S, const double* __restrict__ Pn, int64_t n_rows, int32_t W,
    const uint32_t* __restrict__ mask, double thr, int8_t* __restrict__ out, int32_t* __restrict__ nonneutral,
    int32_t* __restrict__ removed, int32_t* __restrict__ bad) {
    const int64_t row = (int64_t)blockIdx.x * kFiRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (whole wavefronts leave; there is no barrier below)
    fi_filter_row<1, false>(S, Pn, row, W, mask, thr, out, nullptr, nonneutral, removed, bad);
}

}  // namespace icv

// tl.cnv_copy_segments: the level-aware segment tables of the int8 n x W matrix S of copy-number levels
// that tl.cnv_copy_states leaves (0 neutral, -d / +d a loss / gain of distance d), with the mean P(neutral) of every run.
// Integers throughout; the contract (tests/_copy_segments_oracle.py restates it):
//   1. the level range is lo <= 0 <= hi with -7 <= lo and hi <= 7, P = hi - lo + 1 planes; a value outside is flagged.
//   2. runs are those of icv_copy_states_filter: rule 1 of icv_segments.hpp, whose starts and ends compare neighbours for
//      equality (+1 +1 +2 is two runs).  k_seg_rows<.., LEVELS> (icv_segments.hpp) counts and fills them.
//   3. Q[k] = the int64 sum over segment k's windows of q_t = int64(rint(P[i,t] 2^40)): the sum of fi_filter_row
//      (icv_posterior.hpp), so double(Q) / (double(n_windows) 2^40) is the filter's mean, bit for bit.
//   4. counts[g,p,w] (int32) = the cells of group g with level lo + p at window w, the neutral plane included.
//   5. loss / gain = the sums of the planes below / above the neutral one; the sign of the consensus by rule 5 of
//      icv_segments.hpp on them; its magnitude the d in 1 .. (hi or -lo) with the largest counts of level sign d, the
//      smallest such d on a tie.
//   6. group segments = rule 2 on the consensus; cells_min / cells_sum over loss / gain (the cells with the segment's
//      sign), level_min / level_sum over the plane of the segment's level.
//
// Geometry of rule 4: that of k_state_votes (1 024 listed rows x 1 024 columns per workgroup, four adjacent columns per
// thread).  A thread keeps P x 4 counters.  P is a template parameter and the planes are an unrolled chain of
// compare-adds, so the counters are registers: indexed by the level at run time they would live in scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_segments.hpp"  // kVoteRows, kVoteCols, kVoteTile, last_group_at (icv_graph.hpp)

namespace icv {

constexpr int kLevelMax = 7;                    // = ICV_LEVEL_MAX: levels lie in [-7, 7]
constexpr int kLevelPlanes = 2 * kLevelMax + 1;  // the most planes of counts

// rule 4; rows, group_ptr, the tiling and the skipped row numbers as for k_state_votes.  counts: G x P x W, zeroed by
// the caller.  *bad |= 1 where a value that was read lies outside [lo, lo + P - 1].
template <int P>
__global__ __launch_bounds__(256) void k_level_votes(const int8_t* __restrict__ S, int64_t n_rows, int32_t W,
                                                     const int64_t* __restrict__ rows, int64_t M,
                                                     const int64_t* __restrict__ group_ptr, int64_t G,
                                                     uint32_t n_tiles, int32_t lo, int32_t* __restrict__ counts,
                                                     int32_t* __restrict__ bad) {
    const int64_t pos0 = (int64_t)(blockIdx.x / n_tiles) * kVoteRows;
    const int64_t pos1 = pos0 + kVoteRows < M ? pos0 + kVoteRows : M;
    const int64_t c0 = (int64_t)(blockIdx.x % n_tiles) * kVoteTile + (int64_t)threadIdx.x * kVoteCols;
    if (pos0 >= pos1 || c0 >= (int64_t)W) return;
    const bool whole = c0 + kVoteCols <= (int64_t)W;
    int64_t g = last_group_at(group_ptr, G, pos0), pos = pos0;  // the group of position pos0
    bool invalid = false;
    while (pos < pos1 && g < G) {
        int64_t gend = group_ptr[g + 1];
        if (gend <= pos) {  // a group of no rows, or a group_ptr that is not ascending
            ++g;
            continue;
        }
        if (gend > pos1) gend = pos1;
        int32_t cnt[P][kVoteCols];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int j = 0; j < kVoteCols; ++j) cnt[p][j] = 0;
        for (; pos < gend; ++pos) {
            const int64_t r = rows[pos];
            if (r < 0 || r >= n_rows) continue;
            const int8_t* src = S + r * (int64_t)W + c0;
            uint32_t v = 0;
            if (whole) {
                __builtin_memcpy(&v, src, 4);  // (rows are W bytes apart: the four bytes have no alignment)
            } else {
                // (a column past W reads as level 0, which may lie outside no range: lo <= 0 <= hi)
#pragma unroll
                for (int j = 0; j < kVoteCols; ++j)
                    if (c0 + j < (int64_t)W) v |= (uint32_t)(uint8_t)src[j] << (8 * j);
            }
#pragma unroll
            for (int j = 0; j < kVoteCols; ++j) {
                const int u = (int)(int8_t)((v >> (8 * j)) & 0xff) - lo;  // the plane
                invalid |= (unsigned)u >= (unsigned)P;
#pragma unroll
                for (int p = 0; p < P; ++p) cnt[p][j] += u == p;
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            int32_t* dst = counts + (g * P + p) * (int64_t)W + c0;
#pragma unroll
            for (int j = 0; j < kVoteCols; ++j)
                if (c0 + j < (int64_t)W && cnt[p][j]) atomicAdd(dst + j, cnt[p][j]);
        }
        ++g;
    }
    if (invalid) atomicOr(bad, 1);
}

// k_level_votes<planes> for a number of planes known at run time, 1 <= planes <= kLevelPlanes (checked by the caller)
template <int P>
inline void level_votes_launch(int planes, dim3 grid, hipStream_t st, const int8_t* states, int64_t n_rows, int32_t n_cols,
                               const int64_t* rows, int64_t n_listed, const int64_t* group_ptr, int64_t n_groups,
                               uint32_t n_tiles, int32_t lo, int32_t* counts, int32_t* bad) {
    if constexpr (P <= kLevelPlanes) {
        if (planes == P)
            hipLaunchKernelGGL(k_level_votes<P>, grid, dim3(256), 0, st, states, n_rows, n_cols, rows, n_listed, group_ptr,
                               n_groups, n_tiles, lo, counts, bad);
        else
            level_votes_launch<P + 1>(planes, grid, st, states, n_rows, n_cols, rows, n_listed, group_ptr, n_groups, n_tiles,
                                      lo, counts, bad);
    }
}

// rule 5, one thread per group and window; need: int32 per group; counts: G x (hi - lo + 1) x W
__global__ __launch_bounds__(256) void k_level_consensus(const int32_t* __restrict__ counts, const int32_t* __restrict__ need,
                                                         int64_t G, int32_t W, int32_t lo, int32_t hi,
                                                         int32_t* __restrict__ loss, int32_t* __restrict__ gain,
                                                         int8_t* __restrict__ consensus) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= G * (int64_t)W) return;
    const int64_t g = k / W;
    const int32_t* zero = counts + (g * (hi - lo + 1) - lo) * (int64_t)W + (k - g * W);  // the neutral plane's count
    int32_t l = 0, ga = 0, most_l = -1, most_g = -1, dl = 0, dg = 0;
    for (int d = 1; d <= -lo; ++d) {
        const int32_t c = zero[-d * (int64_t)W];
        l += c;
        if (c > most_l) most_l = c, dl = d;  // (strictly more: a tie stays with the smaller d)
    }
    for (int d = 1; d <= hi; ++d) {
        const int32_t c = zero[d * (int64_t)W];
        ga += c;
        if (c > most_g) most_g = c, dg = d;
    }
    const int32_t nd = need[g];
    int c = 0;
    if (ga >= nd && ga > l) c = dg;
    else if (l >= nd && l > ga) c = -dl;
    loss[k] = l;
    gain[k] = ga;
    consensus[k] = (int8_t)c;
}

// rule 6, one thread per group segment.  A segment whose group, windows or level lie outside the tables gets 0 / 0 / 0 / 0.
__global__ __launch_bounds__(256) void k_level_seg_support(
    const int64_t* __restrict__ seg_row, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_end,
    const int8_t* __restrict__ seg_level, int64_t n_seg, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ loss, const int32_t* __restrict__ gain, int64_t G, int32_t W, int32_t lo, int32_t hi,
    int32_t* __restrict__ cells_min, int64_t* __restrict__ cells_sum, int32_t* __restrict__ level_min,
    int64_t* __restrict__ level_sum) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_seg) return;
    const int64_t g = seg_row[k];
    const int32_t s0 = seg_start[k], s1 = seg_end[k];
    const int lv = seg_level[k];
    int32_t smin = 0, lmin = 0;
    int64_t ssum = 0, lsum = 0;
    if (g >= 0 && g < G && s0 >= 0 && s0 < s1 && s1 <= W && lv >= lo && lv <= hi && lv != 0) {
        const int32_t* v = (lv > 0 ? gain : loss) + g * (int64_t)W;
        const int32_t* u = counts + (g * (hi - lo + 1) + (lv - lo)) * (int64_t)W;
        smin = v[s0], lmin = u[s0];
        for (int32_t t = s0; t < s1; ++t) {
            const int32_t a = v[t], b = u[t];
            smin = a < smin ? a : smin;
            lmin = b < lmin ? b : lmin;
            ssum += a;
            lsum += b;
        }
    }
    cells_min[k] = smin, cells_sum[k] = ssum, level_min[k] = lmin, level_sum[k] = lsum;
}

// rule 3, one thread per segment of the per-cell table (seg_row = the row of Pn, n_rows x W float64 row-major without
// padding): psum[k] = Q.  *bad |= 1 where a posterior of a run is not a number in [0, 1] (it counts as 0, as in
// fi_filter_row).  Windows outside the runs are not read and so not validated.  A segment outside the plane gets 0.
// W <= kFiMaxWindows (2^22 terms of at most 2^40 fit an int64); the lanes of a wavefront hold neighbouring runs of one
// row, so the lines they read are shared.
__global__ __launch_bounds__(256) void k_seg_psum(const double* __restrict__ Pn, int64_t n_rows, int32_t W,
                                                  const int64_t* __restrict__ seg_row, const int32_t* __restrict__ seg_start,
                                                  const int32_t* __restrict__ seg_end, int64_t n_seg,
                                                  int64_t* __restrict__ psum, int32_t* __restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_seg) return;
    const int64_t i = seg_row[k];
    const int32_t s0 = seg_start[k], s1 = seg_end[k];
    int64_t sum = 0;
    bool invalid = false;
    if (i >= 0 && i < n_rows && s0 >= 0 && s0 < s1 && s1 <= W) {
        const double* p = Pn + i * (int64_t)W;
        for (int32_t t = s0; t < s1; ++t) {
            const double pv = p[t];
            const bool ok = pv >= 0.0 && pv <= 1.0;  // (false for NaN)
            invalid |= !ok;
            sum += ok ? (int64_t)rint(pv * 1099511627776.0) : 0;
        }
    }
    psum[k] = sum;
    if (invalid) atomicOr(bad, 1);
}

}  // namespace icv

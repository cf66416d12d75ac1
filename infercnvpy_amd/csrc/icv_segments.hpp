// tl.cnv_segments: the altered segments of every cell and of every group of cells, from the int8
// n x W matrix S of loss (-1) / neutral (0) / gain (+1) calls that tl.cnv_states leaves.  Integers throughout; the
// contract (tests/_segments_oracle.py restates it):
//   1. window t of row i STARTS a run iff S[i,t] != 0 and (t is a chromosome start or S[i,t-1] != S[i,t]); it ENDS a run
//      iff S[i,t] != 0 and (t+1 == W or t+1 is a chromosome start or S[i,t+1] != S[i,t]).  The k-th start and the k-th
//      end of a row are segment k: [start, end+1), state S[i,start].
//   2. segments are ordered by row, then by start; offsets[i] (int64) = the number of segments in the rows < i.
//   4. loss[g,w] / gain[g,w] (int32) = the cells of group g with S = -1 / +1 at window w.
//   5. consensus[g,w] = +1 if gain >= need_g and gain > loss; -1 if loss >= need_g and loss > gain; else 0.
//   6. group segments = rules 1-2 on consensus; cells_min / cells_sum = the minimum / the int64 sum over the segment's
//      windows of the winning state's count.
// (Rule 3, min_windows, is a mask on the host.)
//
// Geometry of rules 1-2: one wavefront per row, four rows per 256-thread workgroup.  A wavefront walks its row in steps
// of 1024 windows; each lane takes a strip of 16 consecutive windows as one 16-byte load.  Rows are W bytes apart, so
// the strips are laid out from the 16-byte boundary below the row's first byte: the strips that the row covers only in
// part (its head and its tail) are read byte by byte and never leave the row.  The neighbour byte on either side of a
// strip comes from the adjacent lane (the last lane's from one byte load, the first lane's from the step before), the
// chromosome starts from a bit mask over the windows, built once per call.  A lane's rank among the row's starts (ends)
// is a wavefront prefix sum of the lanes' popcounts plus the running base of the steps before; no lane walks a run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_graph.hpp"

namespace icv {

constexpr int kSegStrip = 16;              // windows per lane and step (one 16-byte load)
constexpr int kSegStep = 64 * kSegStrip;   // windows per wavefront and step
constexpr int kSegRowsPerBlock = 4;        // wavefronts (rows) per workgroup
constexpr int kSegMaskShift = 32;          // bit kSegMaskShift + t of the mask is window t (a head strip starts at t < 0)
constexpr int kVoteRows = 1024;            // entries of `rows` per workgroup of k_state_votes
constexpr int kVoteCols = 4;               // adjacent columns per thread
constexpr int kVoteTile = 256 * kVoteCols; // columns per workgroup

// 32-bit words of the chromosome-start mask of W windows: bits up to kSegMaskShift + W - 1 + kSegStrip are read, two
// words at a time
inline size_t seg_mask_words(int32_t W) { return ((size_t)W + kSegMaskShift + 63) / 32 + 1; }

// mask bit kSegMaskShift + chr_start[c] for the first n_chr entries (the caller zeroes the mask); a start outside
// [0, W) sets nothing
__global__ __launch_bounds__(256) void k_seg_chr_mask(const int32_t* __restrict__ chr_start, int32_t n_chr, int32_t W,
                                                      uint32_t* __restrict__ mask) {
    const int32_t c = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (c >= n_chr) return;
    const int32_t s = chr_start[c];
    if (s < 0 || s >= W) return;
    const uint32_t q = (uint32_t)s + kSegMaskShift;
    atomicOr(&mask[q >> 5], 1u << (q & 31));
}

// rules 1-2.  FILL = false: counts[row] = the row's segments, *bad |= 1 where a value is not -1 / 0 / +1 (LEVELS: where
// it lies outside [lo, hi], the level range of tl.cnv_copy_segments; starts and ends are decided by equality, so the
// rest is the same code, and without LEVELS lo and hi are not read).
// FILL = true: segment offsets[row] + k of the row gets seg_row / seg_start / seg_state from its k-th start and seg_end
// from its k-th end; a position outside [0, n_seg) is not written (offsets that do not belong to S cannot leave the
// tables).  seg_state is the raw byte of S at the start: the fill of level runs is this instantiation.
template <bool FILL, bool LEVELS = false>
__global__ __launch_bounds__(64 * kSegRowsPerBlock) void k_seg_rows(
    const int8_t* __restrict__ S, int64_t n_rows, int32_t W, const uint32_t* __restrict__ mask,
    int64_t* __restrict__ counts, int32_t* __restrict__ bad, const int64_t* __restrict__ offsets, int64_t n_seg,
    int64_t* __restrict__ seg_row, int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_end,
    int8_t* __restrict__ seg_state, int32_t lo, int32_t hi) {
    const int lane = threadIdx.x & 63;
    const int vlo = LEVELS ? lo : -1, vhi = LEVELS ? hi : 1;
    const int64_t row = (int64_t)blockIdx.x * kSegRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (whole wavefronts leave; there is no barrier below)
    const int8_t* p = S + row * (int64_t)W;
    const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(p) & 15);  // bytes from the 16-byte boundary below the row
    const int64_t span = a + (int64_t)W;
    int64_t base = 0;  // FILL: the position of the row's next start; the next end has the same one plus n_end - n_start
    if (FILL) base = offsets[row];
    int64_t n_start = 0, n_end = 0;  // starts / ends of the steps before (FILL), of this lane's strips (count)
    int carry = 0;                   // the byte in front of this step's first strip
    bool invalid = false;

    for (int64_t v0 = 0; v0 < span; v0 += kSegStep) {
        const int64_t t = v0 + lane * kSegStrip - a;  // the window of this strip's first byte: may be < 0 or >= W
        uint64_t lo = 0, hi = 0;                      // the strip, bytes outside the row as 0 (neutral)
        if (t >= 0 && t + kSegStrip <= (int64_t)W) {
            const uint4 q = *reinterpret_cast<const uint4*>(p + t);  // 16-byte aligned: p + t = (p - a) + a multiple of 16
            lo = (uint64_t)q.x | ((uint64_t)q.y << 32);
            hi = (uint64_t)q.z | ((uint64_t)q.w << 32);
        } else if (t + kSegStrip > 0 && t < (int64_t)W) {
#pragma unroll
            for (int j = 0; j < kSegStrip; ++j) {
                const int64_t tt = t + j;
                if (tt >= 0 && tt < (int64_t)W) {
                    const uint64_t b = (uint8_t)p[tt];
                    if (j < 8) lo |= b << (8 * j);
                    else hi |= b << (8 * (j - 8));
                }
            }
        }
        const int first = (int)(int8_t)(lo & 0xff), last = (int)(int8_t)(hi >> 56);
        int prev = __shfl_up(last, 1, 64);
        if (lane == 0) prev = carry;
        int next = __shfl_down(first, 1, 64);
        if (lane == 63) next = (t + kSegStrip < (int64_t)W) ? (int)p[t + kSegStrip] : 0;  // (t >= 0 in lane 63)
        carry = __shfl(last, 63, 64);

        // bit j: window t + j is a chromosome start (j = 0 .. 16)
        uint64_t cs = 0;
        if (t + kSegStrip > 0 && t < (int64_t)W) {
            const int64_t q = t + kSegMaskShift;  // >= kSegMaskShift - 15 > 0
            const uint32_t* m = mask + (q >> 5);
            cs = ((uint64_t)m[0] | ((uint64_t)m[1] << 32)) >> (q & 31);
        }
        uint32_t sf = 0, ef = 0;  // bit j: window t + j starts / ends a run
        int before = prev;
#pragma unroll
        for (int j = 0; j < kSegStrip; ++j) {
            const int s = (int)(int8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xff);
            const int after = j + 1 < kSegStrip
                                  ? (int)(int8_t)((j + 1 < 8 ? lo >> (8 * (j + 1)) : hi >> (8 * (j + 1 - 8))) & 0xff)
                                  : next;
            invalid |= s < vlo || s > vhi;
            if (s != 0) {
                if (((cs >> j) & 1) || before != s) sf |= 1u << j;
                if (((cs >> (j + 1)) & 1) || after != s) ef |= 1u << j;
            }
            before = s;
        }
        if (!FILL) {
            n_start += __popc(sf);
            continue;
        }
        // inclusive wavefront prefix sums of the lanes' starts and ends (at most 16 each: two 16-bit fields)
        const uint32_t mine = (uint32_t)__popc(sf) | ((uint32_t)__popc(ef) << 16);
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const uint32_t excl = incl - mine;
        int64_t ps = base + n_start + (excl & 0xffff), pe = base + n_end + (excl >> 16);
        while (sf) {
            const int j = __ffs(sf) - 1;
            sf &= sf - 1;
            if (ps >= 0 && ps < n_seg) {
                seg_row[ps] = row;
                seg_start[ps] = (int32_t)(t + j);
                seg_state[ps] = (int8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xff);
            }
            ++ps;
        }
        while (ef) {
            const int j = __ffs(ef) - 1;
            ef &= ef - 1;
            if (pe >= 0 && pe < n_seg) seg_end[pe] = (int32_t)(t + j + 1);
            ++pe;
        }
        const uint32_t total = __shfl(incl, 63, 64);
        n_start += total & 0xffff;
        n_end += total >> 16;
    }
    if (!FILL) {
        for (int off = 32; off > 0; off >>= 1) n_start += __shfl_down(n_start, off, 64);
        if (lane == 0) counts[row] = n_start;
        if (__ballot(invalid) != 0 && lane == 0) atomicOr(bad, 1);
    }
}

// rule 4.  rows: M int64 row numbers sorted by group, group_ptr: int64 G + 1 ascending positions from 0 to M.
// Workgroup b takes the kVoteRows entries of `rows` from (b / n_tiles) kVoteRows on and the columns from
// (b % n_tiles) kVoteTile on, four adjacent columns per thread; the counts of one group stay in registers and are added to
// loss / gain (zeroed by the caller) where the group ends or the block does.  Integer sums: the order does not matter.
// A row number outside [0, n_rows) is skipped; *bad |= 1 where a value that was read is not -1 / 0 / +1.
__global__ __launch_bounds__(256) void k_state_votes(const int8_t* __restrict__ S, int64_t n_rows, int32_t W,
                                                     const int64_t* __restrict__ rows, int64_t M,
                                                     const int64_t* __restrict__ group_ptr, int64_t G,
                                                     uint32_t n_tiles, int32_t* __restrict__ loss,
                                                     int32_t* __restrict__ gain, int32_t* __restrict__ bad) {
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
        int32_t nl[kVoteCols] = {0, 0, 0, 0}, ng[kVoteCols] = {0, 0, 0, 0};
        for (; pos < gend; ++pos) {
            const int64_t r = rows[pos];
            if (r < 0 || r >= n_rows) continue;
            const int8_t* src = S + r * (int64_t)W + c0;
            uint32_t v = 0;
            if (whole) {
                __builtin_memcpy(&v, src, 4);  // (rows are W bytes apart: the four bytes have no alignment)
            } else {
#pragma unroll
                for (int j = 0; j < kVoteCols; ++j)
                    if (c0 + j < (int64_t)W) v |= (uint32_t)(uint8_t)src[j] << (8 * j);
            }
#pragma unroll
            for (int j = 0; j < kVoteCols; ++j) {
                const int s = (int)(int8_t)((v >> (8 * j)) & 0xff);
                nl[j] += s == -1;
                ng[j] += s == 1;
                invalid |= s < -1 || s > 1;
            }
        }
        int32_t* lg = loss + g * (int64_t)W + c0;
        int32_t* gg = gain + g * (int64_t)W + c0;
#pragma unroll
        for (int j = 0; j < kVoteCols; ++j) {
            if (c0 + j < (int64_t)W) {
                if (nl[j]) atomicAdd(lg + j, nl[j]);
                if (ng[j]) atomicAdd(gg + j, ng[j]);
            }
        }
        ++g;
    }
    if (invalid) atomicOr(bad, 1);
}

// rule 5, one thread per group and window; need: int32 per group
__global__ __launch_bounds__(256) void k_state_consensus(const int32_t* __restrict__ loss, const int32_t* __restrict__ gain,
                                                         const int32_t* __restrict__ need, int64_t G, int32_t W,
                                                         int8_t* __restrict__ consensus) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= G * (int64_t)W) return;
    const int32_t nd = need[k / W], l = loss[k], g = gain[k];
    int8_t c = 0;
    if (g >= nd && g > l) c = 1;
    else if (l >= nd && l > g) c = -1;
    consensus[k] = c;
}

// rule 6, one thread per group segment: the minimum and the sum over [start, end) of the winning state's count.  A
// segment whose group or windows lie outside the G x W tables gets 0 / 0.
__global__ __launch_bounds__(256) void k_seg_support(const int64_t* __restrict__ seg_row, const int32_t* __restrict__ seg_start,
                                                     const int32_t* __restrict__ seg_end, const int8_t* __restrict__ seg_state,
                                                     int64_t n_seg, const int32_t* __restrict__ loss,
                                                     const int32_t* __restrict__ gain, int64_t G, int32_t W,
                                                     int32_t* __restrict__ cells_min, int64_t* __restrict__ cells_sum) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_seg) return;
    const int64_t g = seg_row[k];
    const int32_t s0 = seg_start[k], s1 = seg_end[k];
    int32_t lo = 0;
    int64_t sum = 0;
    if (g >= 0 && g < G && s0 >= 0 && s0 < s1 && s1 <= W) {
        const int32_t* v = (seg_state[k] > 0 ? gain : loss) + g * (int64_t)W;
        lo = v[s0];
        for (int32_t t = s0; t < s1; ++t) {
            const int32_t c = v[t];
            lo = c < lo ? c : lo;
            sum += c;
        }
    }
    cells_min[k] = lo;
    cells_sum[k] = sum;
}

}  // namespace icv

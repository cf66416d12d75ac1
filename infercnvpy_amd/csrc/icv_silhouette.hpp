// tl.cnv_silhouette: the exact silhouette width of every labelled cell.  The contract
// (tests/_silhouette_oracle.py restates it); x is the n x C representation as float64, 1 <= C <= 256:
//   1. distance: from +0.0, over the components in ascending order, t = x_ic - x_jc, acc = acc + t t (the product rounded
//      before the add, no fma); d_ij = sqrt(acc), correctly rounded.  d_ii is 0 and adds nothing; coincident cells count
//      like any others.
//   2. shift (host): m = the largest |x| over all rows, L = the largest group, b = frexp(m)[1],
//      hc = (bit_length(C - 1) + 1) / 2, e = min(40, 61 - bit_length(L) - (b + 1 + hc)), e = 40 when m == 0.  Since
//      d < 2^(b + 1 + hc), every group sum stays below 2^62.  e < 0 and a non-finite value are errors.
//   3. sums: q_ij = rint(d_ij 2^e) as int64, ties to even; S[i, g] = the int64 sum of q_ij over the cells j of group g, so
//      its order does not matter.  A cell without a label is in no sum.
//   4. means: mean(i, g) = float64(S[i, g]) / (float64(cnt) 2^e), the conversion to nearest even, the divisor exact, one
//      correctly rounded division; cnt = n_g - 1 for the cell's own group and n_g otherwise.
//   5. width: a = the own-group mean (0.0 where the own group is the cell alone), b = the smallest mean over the other
//      groups that have cells, nearest = the lowest group that attains it; s = (b - a) / max(a, b), 0.0 where the own
//      group is the cell alone and where max(a, b) == 0.
// Only float64 subtractions, multiplies, adds, one square root and one division per value in a written order (the
// library is built -ffp-contract=off), and integer sums: the result is a pure function of (x, labels).
//
// Geometry.  The labelled cells are numbered by POSITION: sorted by group, ascending row inside a group (`rows` maps a
// position to its row of x).  The host cuts the positions into j-tiles of at most kSilTileJ cells that never straddle a
// group, and the tiles into consecutive chunks.  A workgroup of 256 threads owns the kSilTileI positions
// [blockIdx.x kSilTileI, + kSilTileI) and the tiles of chunk blockIdx.y.  Per tile it forms the 64 x 64 block of
// distances: thread (ty, tx) of the 16 x 16 holds the 4 x 4 micro-tile of positions i = 4 ty .. + 3, j = 4 tx .. + 3
// in 16 float64 accumulators, and the components go through LDS in stages of kSilTileC, in ascending order, so each
// pair's chain is rule 1 as written and no cell's components are kept in registers: C has no effect on the register
// count.  The thread keeps one int64 running sum per i for the current group; when the next tile belongs to another
// group (the same for the whole workgroup) the 16 threads of an i add theirs up with shuffles and one of them adds the
// sum to S[i, g] with one 64-bit integer atomic: one atomic per (i, group, chunk).  No n x n matrix exists anywhere.
//
// rint(v) for 0 <= v < 2^51 is formed as in icv_tsne.hpp: v + 1.5 2^52 has the unit 1, so the addition IS the rounding
// (ties to even) and the integer is the difference of the bit patterns.  The host entry takes that form (MAGIC) when
// e + (b + 1 + hc) <= 51, and rint and a cast otherwise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icv {

constexpr int kSilThreads = 256;    // 16 x 16 threads, 4 wavefronts
constexpr int kSilTileI = 64;       // positions i per workgroup
constexpr int kSilTileJ = 64;       // positions j per tile
constexpr int kSilTileC = 32;       // components per LDS stage
constexpr int kSilMaxC = 256;       // the cap of pp.neighbors
constexpr int kSilMaxShift = 40;
constexpr int kSilMagicBits = 51;   // MAGIC needs d 2^e < 2^51
constexpr int kSilLd = kSilTileI + 2;  // doubles per component row in LDS: the staging stores of a wavefront spread
                                       // over the banks and a micro-tile's 4 values stay 16-byte aligned
constexpr int kSilFlagNonfinite = 1;
constexpr double kSilMagic = 6755399441055744.0;  // 1.5 2^52
static_assert(kSilTileI == kSilTileJ && kSilTileI == 4 * 16, "a 16 x 16 workgroup of 4 x 4 micro-tiles");

// The tile table, int64 3 x n_tiles: first position, number of positions (1 .. kSilTileJ), group.
// S: int64 (i1 - i0) x n_groups, zeroed by the host entry, for the positions [i0, i1) (i0 a multiple of kSilTileI).
template <typename T, bool MAGIC>
__global__ __launch_bounds__(kSilThreads) void k_sil_sums(
    const T* __restrict__ x, int64_t ld, int64_t n_rows, int C, const int64_t* __restrict__ rows, int64_t n_listed,
    int64_t i0, int64_t i1, const int64_t* __restrict__ tiles, int64_t n_tiles, const int32_t* __restrict__ chunk_ptr,
    int64_t n_groups, double scale, unsigned long long* __restrict__ S, int32_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) double s_i[kSilTileC * kSilLd];
    __shared__ __attribute__((aligned(16))) double s_j[kSilTileC * kSilLd];
    __shared__ int64_t s_row_i[kSilTileI], s_row_j[kSilTileJ];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t ib = i0 + (int64_t)blockIdx.x * kSilTileI;
    // (a row number outside the matrix is never read: the position counts as padding)
    if (tid < kSilTileI) {
        const int64_t p = ib + tid;
        const int64_t r = p < i1 && p < n_listed ? rows[p] : -1;
        s_row_i[tid] = r >= 0 && r < n_rows ? r : -1;
    }
    int64_t t_begin = chunk_ptr[blockIdx.y], t_end = chunk_ptr[blockIdx.y + 1];
    t_begin = t_begin < 0 ? 0 : t_begin;
    t_end = t_end > n_tiles ? n_tiles : t_end;

    unsigned long long run[4] = {0, 0, 0, 0};
    int64_t cur = -1;  // the group of the running sums
    bool nonfinite = false;
    // the running sums of group `cur` go to S (all threads call it together)
    auto flush = [&]() {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            unsigned long long v = run[a];
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1) v += __shfl_xor(v, w, 16);
            const int64_t p = ib + ty * 4 + a;
            if (tx == 0 && p < i1 && p < n_listed && cur >= 0) atomicAdd(&S[(p - i0) * n_groups + cur], v);
            run[a] = 0;
        }
    };

    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t j0 = tiles[t], g = tiles[2 * n_tiles + t];
        int cnt = (int)tiles[n_tiles + t];
        if (g < 0 || g >= n_groups || j0 < 0 || cnt < 1 || cnt > kSilTileJ || j0 + cnt > n_listed) continue;
        if (g != cur) {
            if (cur >= 0) flush();
            cur = g;
        }
        __syncthreads();  // (the last tile's reads of s_row_j and the stages are over)
        if (tid < kSilTileJ) {
            const int64_t r = tid < cnt ? rows[j0 + tid] : -1;
            s_row_j[tid] = r >= 0 && r < n_rows ? r : -1;
        }
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

        for (int c0 = 0; c0 < C; c0 += kSilTileC) {
            const int cc = C - c0 < kSilTileC ? C - c0 : kSilTileC;
            __syncthreads();  // (the row numbers are there; the last stage has been read)
            // stage: lane = component (coalesced along a row of x), 8 cells per pass
            {
                const int c = tid & (kSilTileC - 1);
                for (int cell = tid / kSilTileC; cell < kSilTileI; cell += kSilThreads / kSilTileC) {
                    const int64_t ri = s_row_i[cell], rj = s_row_j[cell];
                    double vi = 0.0, vj = 0.0;
                    if (c < cc) {
                        if (ri >= 0) vi = (double)x[ri * ld + c0 + c];
                        if (rj >= 0) vj = (double)x[rj * ld + c0 + c];
                        nonfinite |= !(fabs(vi) <= 1.7976931348623157e308) || !(fabs(vj) <= 1.7976931348623157e308);
                    }
                    s_i[c * kSilLd + cell] = vi;
                    s_j[c * kSilLd + cell] = vj;
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int c = 0; c < cc; ++c) {
                const double2 i01 = *reinterpret_cast<const double2*>(&s_i[c * kSilLd + ty * 4]);
                const double2 i23 = *reinterpret_cast<const double2*>(&s_i[c * kSilLd + ty * 4 + 2]);
                const double2 j01 = *reinterpret_cast<const double2*>(&s_j[c * kSilLd + tx * 4]);
                const double2 j23 = *reinterpret_cast<const double2*>(&s_j[c * kSilLd + tx * 4 + 2]);
                const double xi[4] = {i01.x, i01.y, i23.x, i23.y}, xj[4] = {j01.x, j01.y, j23.x, j23.y};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const double d = xi[a] - xj[b];
                        acc[a][b] = acc[a][b] + d * d;
                    }
            }
        }
        // rule 3 for the micro-tile (a padding j adds nothing; a padding i is never written)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double v = sqrt(acc[a][b]) * scale;
                unsigned long long q;
                if constexpr (MAGIC)
                    q = (unsigned long long)__double_as_longlong(v + kSilMagic) -
                        (unsigned long long)__double_as_longlong(kSilMagic);
                else
                    q = (unsigned long long)(long long)rint(v);
                run[a] += tx * 4 + b < cnt ? q : 0ull;
            }
    }
    if (cur >= 0) flush();
    if (nonfinite) atomicOr(flags, kSilFlagNonfinite);
}

// Rules 4 and 5, one thread per position p in [i0, i1): its group is found in group_ptr (n_groups + 1 ascending
// positions) by bisection.  s, a, b (float64) and nearest (int32) are indexed by position.
__global__ __launch_bounds__(256) void k_sil_finish(const long long* __restrict__ S, int64_t i0, int64_t i1,
                                                    const int64_t* __restrict__ group_ptr, int64_t n_groups, double scale,
                                                    double* __restrict__ s, double* __restrict__ a_out,
                                                    double* __restrict__ b_out, int32_t* __restrict__ nearest) {
    const int64_t p = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= i1) return;
    int64_t lo = 0, hi = n_groups;  // the last g with group_ptr[g] <= p
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (group_ptr[mid] <= p) lo = mid;
        else hi = mid;
    }
    const int64_t own = lo;
    const long long* row = S + (p - i0) * n_groups;
    double a = 0.0, b = 0.0;
    int64_t at = -1;
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t n_g = group_ptr[g + 1] - group_ptr[g];
        const int64_t cnt = g == own ? n_g - 1 : n_g;
        if (cnt <= 0) continue;
        const double mean = (double)row[g] / ((double)cnt * scale);
        if (g == own) a = mean;
        else if (at < 0 || mean < b) b = mean, at = g;
    }
    const int64_t n_own = group_ptr[own + 1] - group_ptr[own];
    const double top = a > b ? a : b;
    s[p] = n_own <= 1 || top == 0.0 ? 0.0 : (b - a) / top;
    a_out[p] = a;
    b_out[p] = b;
    nearest[p] = (int32_t)at;
}

}  // namespace icv

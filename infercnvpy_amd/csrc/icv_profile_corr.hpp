// tl.cnv_correlation and tl.cnv_signal: Pearson's r of every row of X_cnv with G profiles, and the mean
// square of the row.  The contract (tests/_correlation_oracle.py restates it):
//   1. host, float64: m_g = fsum(p_g) / W, c_g = p_g - m_g, s2_g = fsum(c_g c_g).  The kernel gets c transposed (W x G).
//   2. per row i, sequentially over the windows in ascending order, from +0.0: A += x, B += x x, D_g += x c_g[w]; every
//      product is rounded before its add.  A term with x == 0 adds nothing, so only stored entries are walked and a
//      stored 0.0 or -0.0 changes no bit: CSR and dense rows give the same bits.
//   3. vx = B - (A A) / W; r_g = D_g / sqrt(vx s2_g), clipped to [-1, 1]; NaN where vx <= 0 or s2_g == 0;
//      signal = B / W.  One correctly rounded IEEE operation each.
//   4. best = the lowest g with the largest r that is no NaN; -1 and NaN when the whole row is NaN.
// Only float64 adds, multiplies, one division and one square root in a fixed order; the library is built
// -ffp-contract=off, so the expressions below are evaluated as written.
//
// Geometry: one thread per (row, profile), the profile index fastest.  GP lanes share a row and a wavefront holds 64 / GP
// rows: GP = the power of two >= G, at least 8 and at most 64; without profiles (tl.cnv_signal) GP = 1.  blockIdx.y
// tiles the profiles above 64 (several profiles per lane, so that an entry is handed round once for all of them, were
// measured at 500 profiles and bought nothing: 8.0 to 8.7 ms against 8.8 to 9.0 ms, the table's traffic is what that
// size waits for).  The GP lanes of a row load GP consecutive stored entries (CSR) or windows (dense) of it in one coalesced access
// and hand them round with a shuffle inside the group, so every entry is read from memory once per group; each lane
// then reads its own profile's value at the entry's window: GP contiguous doubles of the W x G table, which is small
// and stays in the caches.  The loads of a whole CSR chunk carry no
// branch (a lane without a profile, or a column outside the matrix, reads element 0 of the table and drops the term), so
// kPcUnroll of them are in flight together.  A dense chunk hands round only its values that are not 0, found by a ballot
// inside the group: zeros add nothing.  With GP = 1 a thread walks its row alone (measured: one profile at GP = 1 took
// 0.48 ms where six at GP = 8 took 0.33 ms, hence the 8).  Every lane keeps A and B as well (the same adds in the same
// order); lane 0 of the first profile tile writes them.  No row is kept in LDS: W and G have no cap.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icv {

constexpr int kPcThreads = 256;   // 4 wavefronts
constexpr int kPcTileG = 64;      // profiles per blockIdx.y
constexpr int kPcUnroll = 8;      // entries of a whole chunk whose profile loads are issued together
constexpr int kPcFlagNonfinite = 1;
constexpr int kPcMinLanes = 8;    // lanes per row from one profile on: a chunk of 8 entries is one 64-byte access

// GP for G profiles: 1 without profiles, else the power of two >= G, at least kPcMinLanes and at most 64
inline int pc_group_lanes(int64_t G) {
    if (G <= 0) return 1;
    int gp = kPcMinLanes;
    while (gp < kPcTileG && gp < G) gp *= 2;
    return gp;
}

template <typename T, bool CSR, int GP>
__global__ __launch_bounds__(kPcThreads) void k_profile_corr(
    const T* __restrict__ val, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t ld,
    int64_t n_rows, int32_t W, const double* __restrict__ ct, const double* __restrict__ s2, int64_t G,
    double* __restrict__ A, double* __restrict__ B, double* __restrict__ signal, double* __restrict__ r,
    int32_t* __restrict__ flags) {
    static_assert(GP >= 1 && GP <= 64 && (GP & (GP - 1)) == 0, "a group is a power of two of lanes inside one wavefront");
    const int gi = threadIdx.x & (GP - 1);
    const int64_t row = (int64_t)blockIdx.x * (kPcThreads / GP) + threadIdx.x / GP;
    if (row >= n_rows) return;  // (whole groups leave: the shuffles below stay inside a group)
    const int64_t g = (int64_t)blockIdx.y * kPcTileG + gi;
    const bool has_g = g < G, any_g = G > 0;  // (this lane has a profile; the table exists)
    const T* src = CSR ? val : val + row * ld;
    const int64_t k_begin = CSR ? indptr[row] : 0, k_end = CSR ? indptr[row + 1] : (int64_t)W;

    double sa = 0.0, sb = 0.0, sd = 0.0;
    bool nonfinite = false;
    // rule 2 for one entry
    auto add = [&](double x, int32_t col) {
        if (!CSR && x == 0.0) return;  // (0.0 and -0.0 add nothing; a NaN goes on)
        nonfinite |= !(fabs(x) <= 1.7976931348623157e308);
        sa = sa + x;
        sb = sb + x * x;
        if (any_g) {
            // (a column outside [0, W) has no profile value: it is passed over)
            const bool use = has_g && (uint32_t)col < (uint32_t)W;
            const double t = sd + x * ct[use ? (int64_t)col * G + g : 0];
            sd = use ? t : sd;
        }
    };

    if constexpr (GP == 1) {
#pragma unroll 4
        for (int64_t k = k_begin; k < k_end; ++k) add((double)src[k], CSR && any_g ? indices[k] : (int32_t)k);
    } else {
        for (int64_t k0 = k_begin; k0 < k_end; k0 += GP) {
            // lane gi of the group holds entry k0 + gi and hands it round
            const int64_t k = k0 + gi;
            double mine = 0.0;
            int32_t mine_col = 0;
            if (k < k_end) {
                mine = (double)src[k];
                mine_col = CSR ? indices[k] : (int32_t)k;
            }
            if constexpr (!CSR) {
                // a dense chunk is mostly zeros: only the lanes of the group whose value is not 0, in window order
                // (the lanes of a group hold the same mask, so they stay together)
                constexpr unsigned long long kGroup = GP == 64 ? ~0ull : (1ull << (GP & 63)) - 1;
                unsigned long long todo = (__ballot(mine != 0.0) >> ((threadIdx.x & 63) & ~(GP - 1))) & kGroup;
                while (todo) {
                    const int j = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    add(__shfl(mine, j, GP), __shfl(mine_col, j, GP));
                }
            } else if (k_end - k0 >= GP) {  // a whole chunk: constant trip counts
                constexpr int U = GP < kPcUnroll ? GP : kPcUnroll;
                for (int j0 = 0; j0 < GP; j0 += U) {
#pragma unroll
                    for (int u = 0; u < U; ++u) add(__shfl(mine, j0 + u, GP), __shfl(mine_col, j0 + u, GP));
                }
            } else {
                const int cnt = (int)(k_end - k0);
                for (int j = 0; j < cnt; ++j) add(__shfl(mine, j, GP), __shfl(mine_col, j, GP));
            }
        }
    }

    if (gi == 0 && blockIdx.y == 0) {
        A[row] = sa;
        B[row] = sb;
        signal[row] = sb / (double)W;
        if (nonfinite) atomicOr(flags, kPcFlagNonfinite);
    }
    if (has_g) {
        const double vx = sb - (sa * sa) / (double)W;
        const double sg = s2[g];
        double c = __longlong_as_double(0x7ff8000000000000LL);
        if (vx > 0.0 && sg != 0.0) {
            c = sd / sqrt(vx * sg);
            c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);  // (a NaN stays)
        }
        r[row * G + g] = c;
    }
}

// rule 4, one thread per row of r
__global__ __launch_bounds__(256) void k_profile_corr_best(const double* __restrict__ r, int64_t n_rows, int64_t G,
                                                           double* __restrict__ best_r, int32_t* __restrict__ best_g) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const double* p = r + row * G;
    double best = __longlong_as_double(0x7ff8000000000000LL);
    int32_t at = -1;
    for (int64_t g = 0; g < G; ++g) {
        const double v = p[g];
        if (v == v && (at < 0 || v > best)) {
            best = v;
            at = (int32_t)g;
        }
    }
    best_r[row] = best;
    best_g[row] = at;
}

}  // namespace icv

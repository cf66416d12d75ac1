// tl.cnv_kmeans: deterministic exact k-means of the n x C representation.  The contract
// (tests/_kmeans_oracle.py restates it); x is used as float64, 1 <= C <= 256, 2 <= k <= 256, k <= n:
//   1. squared distance: from +0.0, over the components in ascending order, t = x_ic - c_gc, acc = acc + t t (the product
//      rounded before the add, no fma); D(i, g) = acc.  No square root is taken.
//   2. shifts (host): m = the largest |value| of x and of a given table of centres, b = frexp(m)[1],
//      e = min(40, 62 - bit_length(n) - b) for coordinates (|rint(x 2^e)| <= 2^(b + e): a sum over n cells stays within
//      int64), f = min(40, 61 - bit_length(n) - (2b + 2 + bit_length(C - 1))) for squared distances
//      (D < 2^(2b + 2 + bit_length(C - 1))); both 40 when m == 0.  e < 0, f < 0 and a non-finite value are errors.
//   3. hash (host): z_t = mix(base_r ^ t), base_r = mix(((random_state + r) mod 2^64) ^ mix(TAG)), mix = splitmix64's
//      finaliser.  The kernels only see z_t.
//   4. seeding: centre 0 is row z_0 mod n.  For t = 1 .. k - 1: w_i = rint(min_{g < t} D(i, g) 2^f) as int64, ties to even;
//      P the inclusive prefix sum of w in row order, W = P_{n-1}, theta = z_t mod W; centre t is the first row i with
//      P_i > theta, taken as the float64 row itself.  W == 0 (fewer than t + 1 distinct points) is an error.
//   5. assignment: label_i = the lowest g that attains min_g D(i, g); n_changed = the labels that differ from the ones
//      found there (the caller fills them with -1 before iteration 1); I = the int64 sum of rint(D(i, label_i) 2^f).
//   6. update: q_ic = rint(x_ic 2^e) as int64, Q[g, c] = the int64 sum of q_ic over the cells of g, n_g their number;
//      c_gc = float64(Q[g, c]) / (float64(n_g) 2^e): one conversion to nearest even, an exact divisor, one correctly rounded
//      division.  A cluster without cells keeps its centre.
// Rules 7 and 8 (the loop and the restarts) are the host's.  Only float64 subtractions, multiplies, adds and one division in
// a written order (the library is built -ffp-contract=off) and integer sums: the result is a pure function of the input.
//
// Geometry.  Assignment: a workgroup of 256 threads owns kKmTileCells cells and walks the centres in tiles of
// kKmTileCentres, ascending.  Thread (ty, tx) of the 64 x 4 holds the 4 x 4 micro-tile of cells 4 ty .. + 3 and centres
// 4 tx .. + 3 in 16 float64 accumulators; the components go through LDS in stages of kKmTileC, ascending, so every chain is
// rule 1 as written and C has no effect on the register count.  After a tile the 4 lanes of a cell take a (value, index)
// minimum and the running best takes it with a strict <, so ties go to the lowest g within and across tiles.  One 64-bit
// atomic per workgroup for I and one for n_changed.
// Update: a workgroup per (slab of kKmUpdRows rows, tile of kKmUpdTileC components) keeps k x kKmUpdTileC int64 sums in
// LDS (64-bit LDS atomics) and adds one global 64-bit atomic per non-zero (slab, g, c); the component tile 0 counts the cells.
// Seeding: one thread per row forms D(i, t - 1), the running minimum and w_i; a workgroup writes one partial sum of w, no
// atomics.  The one-workgroup pick totals the partials, forms theta, finds the block, then the row (w >= 0, so exactly one
// block and one row have prefix - w <= theta < prefix), and copies the row into the table of centres.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icv {

constexpr int kKmThreads = 256;      // 4 wavefronts
constexpr int kKmTileCells = 256;    // cells per workgroup of the assignment: 64 x 4 per thread
constexpr int kKmTileCentres = 16;   // centres per tile: 4 x 4 per thread
constexpr int kKmTileC = 32;         // components per LDS stage
constexpr int kKmMaxC = 256;         // the cap of pp.neighbors
constexpr int kKmMaxK = 256;
constexpr int kKmMaxShift = 40;
constexpr int kKmSeedRows = 256;     // rows per partial sum of the seeding weights
constexpr int kKmUpdRows = 1024;     // rows per slab of the update
constexpr int kKmUpdTileC = 16;      // components per workgroup of the update: k x 16 int64 in LDS
constexpr int kKmLdX = kKmTileCells + 2;  // doubles per component row of the cell tile in LDS (as kSilLd)
constexpr int kKmFlagNonfinite = 1, kKmFlagNoMass = 2;
static_assert(kKmTileCells == 4 * (kKmThreads / 4) && kKmTileCentres == 4 * 4, "64 x 4 threads of 4 x 4 micro-tiles");
static_assert(kKmSeedRows == kKmThreads && kKmMaxC <= kKmThreads, "one thread per row; one per component of a centre");

__device__ __forceinline__ bool km_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }

// the sum of v over the workgroup, in every thread (s_red: 4 slots)
__device__ __forceinline__ unsigned long long km_block_sum(unsigned long long v, unsigned long long* s_red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();  // (the last use of s_red is over)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// the inclusive prefix sum of v over the threads of the workgroup (s_scan: kKmThreads slots; s_scan[kKmThreads - 1] is
// the total until the next barrier-protected write)
__device__ __forceinline__ unsigned long long km_block_scan(unsigned long long v, unsigned long long* s_scan) {
    const int tid = threadIdx.x;
    s_scan[tid] = v;
    __syncthreads();
    for (int off = 1; off < kKmThreads; off <<= 1) {
        const unsigned long long t = tid >= off ? s_scan[tid - off] : 0ull;
        __syncthreads();
        s_scan[tid] += t;
        __syncthreads();
    }
    return s_scan[tid];
}

// Rule 4's weights for the centre that was picked last (`centre`, C float64): mind_i = D(i, centre), or its minimum with
// the value found there unless `first`; w_i = rint(mind_i 2^f); partials[blockIdx.x] = the sum of w over the block's rows.
template <typename T>
__global__ __launch_bounds__(kKmThreads) void k_km_seed_dist(const T* __restrict__ x, int64_t ld, int64_t n, int C,
                                                             const double* __restrict__ centre, int first, double scale_f,
                                                             double* __restrict__ mind, long long* __restrict__ w,
                                                             unsigned long long* __restrict__ partials,
                                                             int32_t* __restrict__ flags) {
    __shared__ double s_c[kKmMaxC];
    __shared__ unsigned long long s_red[4];
    if ((int)threadIdx.x < C) s_c[threadIdx.x] = centre[threadIdx.x];
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * kKmSeedRows + threadIdx.x;
    unsigned long long wi = 0;
    if (row < n) {
        const T* p = x + row * ld;
        double acc = 0.0;
        for (int c = 0; c < C; ++c) {
            const double t = (double)p[c] - s_c[c];
            acc = acc + t * t;
        }
        if (!km_finite(acc)) atomicOr(flags, kKmFlagNonfinite);
        if (!first) {
            const double m = mind[row];
            acc = m < acc ? m : acc;
        }
        mind[row] = acc;
        const long long q = __double2ll_rn(acc * scale_f);
        w[row] = q;
        wi = (unsigned long long)q;
    }
    const unsigned long long total = km_block_sum(wi, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Rule 4's draw for centre t, one workgroup: the row is z mod n for t == 0, otherwise the first row whose inclusive prefix
// sum of w exceeds theta = z mod W.  The row's values become centres[t C ..] and picks[t] its number; W == 0 sets
// kKmFlagNoMass, picks[t] = -1 and leaves the centre alone.
template <typename T>
__global__ __launch_bounds__(kKmThreads) void k_km_seed_pick(const T* __restrict__ x, int64_t ld, int64_t n, int C,
                                                             const long long* __restrict__ w,
                                                             const unsigned long long* __restrict__ partials,
                                                             int64_t n_blocks, int t, unsigned long long z,
                                                             double* __restrict__ centres, int64_t* __restrict__ picks,
                                                             int32_t* __restrict__ flags) {
    __shared__ unsigned long long s_scan[kKmThreads];
    __shared__ unsigned long long s_base;
    __shared__ int64_t s_block, s_row;
    const int tid = threadIdx.x;
    int64_t row;
    if (t == 0) {
        row = (int64_t)(z % (unsigned long long)n);
    } else {
        if (tid == 0) s_base = 0, s_block = 0, s_row = 0;
        // the partial sums in 256 consecutive chunks, one per thread
        const int64_t per = (n_blocks + kKmThreads - 1) / kKmThreads;
        const int64_t lo = tid * per < n_blocks ? tid * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
        unsigned long long mine = 0;
        for (int64_t b = lo; b < hi; ++b) mine += partials[b];
        const unsigned long long incl = km_block_scan(mine, s_scan);
        const unsigned long long total = s_scan[kKmThreads - 1];
        if (total == 0) {  // (the whole workgroup)
            if (tid == 0) {
                picks[t] = -1;
                atomicOr(flags, kKmFlagNoMass);
            }
            return;
        }
        const unsigned long long theta = z % total;
        if (incl - mine <= theta && theta < incl) {  // (one thread: the sums are not negative)
            unsigned long long run = incl - mine;
            for (int64_t b = lo; b < hi; ++b) {
                const unsigned long long p = partials[b];
                if (theta < run + p) {
                    s_block = b;
                    s_base = run;
                    break;
                }
                run += p;
            }
        }
        __syncthreads();
        const unsigned long long base = s_base;
        const int64_t r = s_block * kKmSeedRows + tid;
        const unsigned long long wi = r < n ? (unsigned long long)w[r] : 0ull;
        const unsigned long long at = base + km_block_scan(wi, s_scan);
        if (at - wi <= theta && theta < at) s_row = r;  // (one thread)
        __syncthreads();
        row = s_row;
    }
    row = row < 0 ? 0 : (row < n ? row : n - 1);  // (w of non-finite values: the flag says so; never out of the matrix)
    if (tid < C) centres[(int64_t)t * C + tid] = (double)x[row * ld + tid];
    if (tid == 0) picks[t] = row;
}

// Rule 5 for the cells [blockIdx.x kKmTileCells, + kKmTileCells): labels (read for n_changed, then written), sqdist =
// D(i, label_i); stats[0] += the inertia terms, stats[1] += the labels that changed.
template <typename T>
__global__ __launch_bounds__(kKmThreads) void k_km_assign(const T* __restrict__ x, int64_t ld, int64_t n, int C,
                                                          const double* __restrict__ centres, int k, double scale_f,
                                                          int32_t* __restrict__ labels, double* __restrict__ sqdist,
                                                          unsigned long long* __restrict__ stats,
                                                          int32_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) double s_x[kKmTileC * kKmLdX];
    __shared__ __attribute__((aligned(16))) double s_c[kKmTileC * kKmTileCentres];
    __shared__ unsigned long long s_red[4];
    const int tid = threadIdx.x, tx = tid & 3, ty = tid >> 2;
    const int64_t i0 = (int64_t)blockIdx.x * kKmTileCells;
    double best[4];
    int best_g[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) best[a] = __builtin_inf(), best_g[a] = 0;
    bool nonfinite = false;

    for (int g0 = 0; g0 < k; g0 += kKmTileCentres) {
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        for (int c0 = 0; c0 < C; c0 += kKmTileC) {
            const int cc = C - c0 < kKmTileC ? C - c0 : kKmTileC;
            __syncthreads();  // (the last stage has been read)
            // stage: lane = component (coalesced along a row of x), 8 cells per pass; then the tile of centres
            {
                const int c = tid & (kKmTileC - 1);
                for (int cell = tid / kKmTileC; cell < kKmTileCells; cell += kKmThreads / kKmTileC) {
                    const int64_t r = i0 + cell;
                    double v = 0.0;
                    if (c < cc && r < n) {
                        v = (double)x[r * ld + c0 + c];
                        nonfinite |= !km_finite(v);
                    }
                    s_x[c * kKmLdX + cell] = v;
                }
                for (int at = tid; at < kKmTileC * kKmTileCentres; at += kKmThreads) {
                    const int cs = at & (kKmTileC - 1), g = at / kKmTileC;
                    s_c[cs * kKmTileCentres + g] = cs < cc && g0 + g < k ? centres[(int64_t)(g0 + g) * C + c0 + cs] : 0.0;
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int c = 0; c < cc; ++c) {
                const double2 i01 = *reinterpret_cast<const double2*>(&s_x[c * kKmLdX + ty * 4]);
                const double2 i23 = *reinterpret_cast<const double2*>(&s_x[c * kKmLdX + ty * 4 + 2]);
                const double2 j01 = *reinterpret_cast<const double2*>(&s_c[c * kKmTileCentres + tx * 4]);
                const double2 j23 = *reinterpret_cast<const double2*>(&s_c[c * kKmTileCentres + tx * 4 + 2]);
                const double xi[4] = {i01.x, i01.y, i23.x, i23.y}, cj[4] = {j01.x, j01.y, j23.x, j23.y};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const double d = xi[a] - cj[b];
                        acc[a][b] = acc[a][b] + d * d;
                    }
            }
        }
        // the tile's (value, index) minimum per cell: ascending inside the thread, then across the 4 lanes of the cell
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double v = __builtin_inf();
            int g = kKmMaxK;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int gb = g0 + tx * 4 + b;
                if (gb < k && acc[a][b] < v) v = acc[a][b], g = gb;
            }
#pragma unroll
            for (int d = 1; d <= 2; d <<= 1) {
                const double ov = __shfl_xor(v, d, 4);
                const int og = __shfl_xor(g, d, 4);
                if (ov < v || (ov == v && og < g)) v = ov, g = og;
            }
            if (v < best[a]) best[a] = v, best_g[a] = g;
        }
    }

    unsigned long long inertia = 0, changed = 0;
    if (tx == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int64_t r = i0 + ty * 4 + a;
            if (r < n) {
                changed += labels[r] != best_g[a];
                labels[r] = best_g[a];
                sqdist[r] = best[a];
                inertia += (unsigned long long)__double2ll_rn(best[a] * scale_f);
            }
        }
    }
    inertia = km_block_sum(inertia, s_red);
    changed = km_block_sum(changed, s_red);
    if (tid == 0) {
        atomicAdd(&stats[0], inertia);
        if (changed) atomicAdd(&stats[1], changed);
    }
    if (nonfinite) atomicOr(flags, kKmFlagNonfinite);
}

// Rule 6's sums for the rows [blockIdx.x kKmUpdRows, + kKmUpdRows) and the components [blockIdx.y kKmUpdTileC,
// + kKmUpdTileC): Q (k x C) and, from the component tile 0, counts (k).  A label outside [0, k) is in no sum.
template <typename T>
__global__ __launch_bounds__(kKmThreads) void k_km_update(const T* __restrict__ x, int64_t ld, int64_t n, int C,
                                                          const int32_t* __restrict__ labels, int k, double scale_e,
                                                          unsigned long long* __restrict__ Q,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long s_q[kKmMaxK * kKmUpdTileC];
    __shared__ unsigned int s_n[kKmMaxK];
    const int tid = threadIdx.x;
    for (int at = tid; at < k * kKmUpdTileC; at += kKmThreads) s_q[at] = 0;
    for (int g = tid; g < k; g += kKmThreads) s_n[g] = 0;
    __syncthreads();
    const int c = tid & (kKmUpdTileC - 1), col = (int)blockIdx.y * kKmUpdTileC + c;
    const int64_t r0 = (int64_t)blockIdx.x * kKmUpdRows, r1 = r0 + kKmUpdRows < n ? r0 + kKmUpdRows : n;
    for (int64_t r = r0 + tid / kKmUpdTileC; r < r1; r += kKmThreads / kKmUpdTileC) {
        const int g = labels[r];
        if (g < 0 || g >= k) continue;
        if (col < C) {
            const long long q = __double2ll_rn((double)x[r * ld + col] * scale_e);
            if (q != 0) atomicAdd(&s_q[g * kKmUpdTileC + c], (unsigned long long)q);
        }
        if (blockIdx.y == 0 && c == 0) atomicAdd(&s_n[g], 1u);
    }
    __syncthreads();
    for (int at = tid; at < k * kKmUpdTileC; at += kKmThreads) {
        const int g = at / kKmUpdTileC, cq = (int)blockIdx.y * kKmUpdTileC + (at & (kKmUpdTileC - 1));
        const unsigned long long v = s_q[at];
        if (v != 0 && cq < C) atomicAdd(&Q[(int64_t)g * C + cq], v);
    }
    if (blockIdx.y == 0)
        for (int g = tid; g < k; g += kKmThreads)
            if (s_n[g]) atomicAdd(&counts[g], (unsigned long long)s_n[g]);
}

// Rule 6's division, one thread per (g, c); a cluster without cells keeps its centre.
__global__ __launch_bounds__(kKmThreads) void k_km_centres(const long long* __restrict__ Q,
                                                           const long long* __restrict__ counts, int k, int C,
                                                           double scale_e, double* __restrict__ centres) {
    const int at = (int)blockIdx.x * kKmThreads + threadIdx.x;
    if (at >= k * C) return;
    const long long n_g = counts[at / C];
    if (n_g > 0) centres[at] = __ll2double_rn(Q[at]) / (__ll2double_rn(n_g) * scale_e);
}

}  // namespace icv

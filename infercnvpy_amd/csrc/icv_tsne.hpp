// tl.tsne: sklearn's sparse affinities, the EXACT repulsion over all ordered pairs and the update rules
// of sklearn's _gradient_descent.  Every sum over pairs or entries is an int64 sum of contributions rounded to a
// multiple of 2^-32 (repulsion) or 2^-40 (attraction), so it does not depend on tiling, lanes or atomics, and every
// other operation is one correctly rounded IEEE operation in a written order (the library is built
// -ffp-contract=off): an iteration equals tests/_tsne_oracle.py bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_graph.hpp"  // ld_wave_sum, kGraphLongRow, k_graph_check (the validation)

namespace icv {

constexpr int kTsLongRow = kGraphLongRow;      // rows above this many entries take a workgroup in k_ts_step
constexpr int kTsTile = 256;                   // positions per LDS tile of k_ts_repulse (= its block size)
constexpr int64_t kTsMaxRow = (int64_t)1 << 22;  // |attraction term| 2^40 <= 2^40: 2^22 of them fit an int64

// ---- rule 2: the written exponential (0 below -708; Taylor degree 13 after the reduction by k ln 2) ---------------------
__device__ __forceinline__ double ts_exp(double x) {
    if (!(x >= -708.0)) return 0.0;
    const double k = rint(x * 1.4426950408889634);
    const double r = (x - k * 0x1.62e42fee00000p-1) - k * 1.9082149292705877e-10;
    double p = 1.6059043836821613e-10;
    p = p * r + 2.08767569878681e-09;
    p = p * r + 2.505210838544172e-08;
    p = p * r + 2.755731922398589e-07;
    p = p * r + 2.7557319223985893e-06;
    p = p * r + 2.48015873015873e-05;
    p = p * r + 0.0001984126984126984;
    p = p * r + 0.001388888888888889;
    p = p * r + 0.008333333333333333;
    p = p * r + 0.041666666666666664;
    p = p * r + 0.16666666666666666;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return ldexp(p, (int)k);
}

// is the entropy of the row at beta above log(perplexity) = target?
__device__ __forceinline__ bool ts_above(const float* __restrict__ dr, int kk, double d0, double beta, double target) {
    double S = 0.0, E = 0.0;
    for (int r = 0; r < kk; ++r) {
        const double d = (double)dr[r];
        const double rel = d * d - d0;
        const double e = ts_exp(-(beta * rel));
        S += e;
        E += rel * e;
    }
    return S > ts_exp(target - (beta * E) / S);
}

// One lane per row: beta by the fixed bisection, then the conditional affinities p (n x kk, float64)
__global__ void __launch_bounds__(256) k_ts_affinity(const float* __restrict__ dist, int64_t n, int kk, double target,
                                                     double* __restrict__ beta_out, double* __restrict__ p_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* dr = dist + i * kk;
    const double d0 = (double)dr[0] * (double)dr[0];
    const double dl = (double)dr[kk - 1] * (double)dr[kk - 1];
    if (dl - d0 == 0.0) {  // all distances equal
        beta_out[i] = 1.0;
        for (int r = 0; r < kk; ++r) p_out[i * kk + r] = 1.0 / (double)kk;
        return;
    }
    const double inf = (double)__builtin_huge_valf();
    double lo = 0.0, hi = inf, beta = 1.0;
    bool found = false;
    for (int step = 0; step < 64; ++step) {
        const bool up = ts_above(dr, kk, d0, beta, target);
        if (up) lo = beta;
        else hi = beta;
        if (lo > 0.0 && hi < inf) {
            found = true;
            break;
        }
        if (step < 63) beta = up ? beta * 2.0 : beta / 2.0;
    }
    if (found) {
        for (int it = 0; it < 64; ++it) {
            const double mid = (lo + hi) / 2.0;
            if (ts_above(dr, kk, d0, mid, target)) lo = mid;
            else hi = mid;
        }
        beta = (lo + hi) / 2.0;
    }
    double S = 0.0;
    for (int r = 0; r < kk; ++r) {
        const double d = (double)dr[r];
        S += ts_exp(-(beta * (d * d - d0)));
    }
    beta_out[i] = beta;
    for (int r = 0; r < kk; ++r) {
        const double d = (double)dr[r];
        p_out[i * kk + r] = ts_exp(-(beta * (d * d - d0))) / S;
    }
}

// ---- rule 4: the repulsion ------------------------------------------------------------------------------------------------
// v (|v| < 2^19) + 1.5 2^20 in float64 has the unit 2^-32: the addition IS rint(v 2^32) (ties to even), and the integer
// is the difference of the bit patterns.  The kernel adds the patterns and takes the constant out once at the end
// (unsigned arithmetic: the sums wrap, the final differences are the signed values).
constexpr double kTsMagic = 1572864.0;
__device__ __forceinline__ unsigned long long ts_bits(float v) {
    return (unsigned long long)__double_as_longlong((double)v + kTsMagic);
}

// A thread owns cell i = blockIdx.x * 256 + threadIdx.x; the workgroup streams the positions [blockIdx.y * chunk,
// + chunk) through LDS in tiles of kTsTile (every lane reads the same address: a broadcast) and adds its partial sums
// to zr[i], rr[i * C + c] with integer atomics.  The pair (i, i) is taken out BY INDEX: its terms are rint(2^32) and
// 0 whatever the position, and they are subtracted when i lies in the chunk (cells at the same place as i count with
// q = 1).  The last workgroup of a column of the grid to finish (ticket) reads the complete zr of its 256 cells and
// adds their halves to hl[0] (high) and hl[1] (low).
template <int C>
__global__ __launch_bounds__(256) void k_ts_repulse(const float* __restrict__ y, int64_t n, int64_t chunk,
                                                    unsigned long long* __restrict__ zr, unsigned long long* __restrict__ rr,
                                                    unsigned long long* __restrict__ hl, unsigned* __restrict__ ticket) {
    __shared__ float s_y[kTsTile * C];
    __shared__ long long s_red[2][4];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool valid = i < n;
    float yi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) yi[c] = valid ? y[i * C + c] : 0.f;
    const int64_t j0 = (int64_t)blockIdx.y * chunk;
    const int64_t j1 = j0 + chunk < n ? j0 + chunk : n;
    unsigned long long az = 0, ar[C];
#pragma unroll
    for (int c = 0; c < C; ++c) ar[c] = 0;
    for (int64_t jt = j0; jt < j1; jt += kTsTile) {
        const int m = (int)(j1 - jt < kTsTile ? j1 - jt : kTsTile);
        __syncthreads();
        for (int e = tid; e < m * C; e += 256) s_y[e] = y[jt * C + e];
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < m; ++jj) {
            float dx[C];
#pragma unroll
            for (int c = 0; c < C; ++c) dx[c] = yi[c] - s_y[jj * C + c];
            float d2 = dx[0] * dx[0] + dx[1] * dx[1];
            if (C == 3) d2 = d2 + dx[2] * dx[2];
            const float q = 1.0f / (1.0f + d2);
            const float qq = q * q;
            az += ts_bits(q);
#pragma unroll
            for (int c = 0; c < C; ++c) ar[c] += ts_bits(qq * dx[c]);
        }
    }
    const unsigned long long base = (unsigned long long)(j1 - j0) * (unsigned long long)__double_as_longlong(kTsMagic);
    az -= base;
    if (i >= j0 && i < j1) az -= 4294967296ull;  // the pair (i, i)
    if (valid) {
        atomicAdd(&zr[i], az);
#pragma unroll
        for (int c = 0; c < C; ++c) atomicAdd(&rr[i * C + c], ar[c] - base);
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(&ticket[blockIdx.x], 1u) == gridDim.y - 1;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    long long hi = 0, lo = 0;
    if (valid) {
        const unsigned long long z = __hip_atomic_load(&zr[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        hi = (long long)(z >> 32), lo = (long long)(z & 0xffffffffull);
    }
    hi = ld_wave_sum(hi), lo = ld_wave_sum(lo);
    if ((tid & 63) == 0) s_red[0][tid >> 6] = hi, s_red[1][tid >> 6] = lo;
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&hl[0], (unsigned long long)(s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3]));
        atomicAdd(&hl[1], (unsigned long long)(s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3]));
        ticket[blockIdx.x] = 0;  // for the next iteration
    }
}

// ---- rules 5 and 6 ------------------------------------------------------------------------------------------------------------
struct TsStep {
    double coef;  // ex_t / (2 n)
    double mom;   // m_t
    double eta;   // learning_rate
    int64_t n;
};

template <int C>
__device__ __forceinline__ void ts_attract(const float* __restrict__ y, const double (&yi)[C], int64_t j, float wf,
                                           long long (&acc)[C]) {
    double d[C];
    double d2 = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        d[c] = yi[c] - (double)y[j * C + c];
        d2 = c == 0 ? d[c] * d[c] : d2 + d[c] * d[c];
    }
    const double wq = (double)wf * (1.0 / (1.0 + d2));
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += __double2ll_rn((wq * d[c]) * 1099511627776.0);
}

// coordinate c of cell v: the gradient, the gain, the update and the new position; the accumulators of the NEXT
// iteration (the other set) are zeroed on the way
__device__ __forceinline__ void ts_update(int64_t at, long long A, const unsigned long long* __restrict__ rr,
                                          const unsigned long long* __restrict__ hl, const TsStep& P,
                                          const float* __restrict__ y, const float* __restrict__ u,
                                          const float* __restrict__ gain, float* __restrict__ y_out, float* __restrict__ u_out,
                                          float* __restrict__ gain_out) {
    const double Z = (double)(long long)hl[0] + (double)(long long)hl[1] * (1.0 / 4294967296.0);
    const double rep = Z > 0.0 ? ((double)(long long)rr[at] * (1.0 / 4294967296.0)) / Z : 0.0;
    const double g = 4.0 * (P.coef * ((double)A * (1.0 / 1099511627776.0)) - rep);
    const double ud = (double)u[at], gd = (double)gain[at];
    double gn = ud * g < 0.0 ? gd + 0.2 : gd * 0.8;
    gn = gn < 0.01 ? 0.01 : gn;  // (a NaN stays a NaN, as numpy's maximum)
    const float gf = (float)gn;
    const float uf = (float)(P.mom * ud - P.eta * ((double)gf * g));
    gain_out[at] = gf;
    u_out[at] = uf;
    y_out[at] = (float)((double)y[at] + (double)uf);
}

// Blocks [0, short_blocks): a wavefront per row, 4 rows per block (rows above kTsLongRow entries are left to the blocks
// from short_blocks on: a workgroup per row of long_list).  zr_next / rr_next / hl_next: the accumulators that the
// repulsion of the next iteration adds to.
template <int C>
__global__ __launch_bounds__(256) void k_ts_step(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                 const float* __restrict__ val, const int32_t* __restrict__ long_list,
                                                 unsigned short_blocks, TsStep P, const unsigned long long* __restrict__ rr,
                                                 const unsigned long long* __restrict__ hl,
                                                 unsigned long long* __restrict__ zr_next,
                                                 unsigned long long* __restrict__ rr_next,
                                                 unsigned long long* __restrict__ hl_next, const float* __restrict__ y,
                                                 const float* __restrict__ u, const float* __restrict__ gain,
                                                 float* __restrict__ y_out, float* __restrict__ u_out,
                                                 float* __restrict__ gain_out) {
    __shared__ long long s_acc[4][C];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 2) hl_next[threadIdx.x] = 0;

    if (blockIdx.x >= short_blocks) {  // ---- a long row
        const int64_t v = long_list[blockIdx.x - short_blocks];
        const int64_t b = indptr[v], e = indptr[v + 1];
        double yi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) yi[c] = (double)y[v * C + c];
        for (int64_t it = b + threadIdx.x; it < e; it += 256) ts_attract<C>(y, yi, col[it], val[it], acc);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = ld_wave_sum(acc[c]);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) s_acc[wave][c] = acc[c];
        }
        __syncthreads();
        if (threadIdx.x < C) {
            const int c = threadIdx.x;
            ts_update(v * C + c, s_acc[0][c] + s_acc[1][c] + s_acc[2][c] + s_acc[3][c], rr, hl, P, y, u, gain, y_out,
                      u_out, gain_out);
            rr_next[v * C + c] = 0;
            if (c == 0) zr_next[v] = 0;
        }
        return;
    }

    // ---- a short row per wavefront
    const int64_t v = (int64_t)blockIdx.x * 4 + wave;
    if (v >= P.n) return;
    const int64_t b = indptr[v], e = indptr[v + 1];
    if (e - b > kTsLongRow) return;
    double yi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) yi[c] = (double)y[v * C + c];
    for (int64_t it = b + lane; it < e; it += 64) ts_attract<C>(y, yi, col[it], val[it], acc);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const long long A = ld_wave_sum(acc[c]);
        if (lane == c) {
            ts_update(v * C + c, A, rr, hl, P, y, u, gain, y_out, u_out, gain_out);
            rr_next[v * C + c] = 0;
            if (c == 0) zr_next[v] = 0;
        }
    }
}

}  // namespace icv

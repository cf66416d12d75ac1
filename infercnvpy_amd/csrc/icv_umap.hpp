// tl.umap: one epoch of the gather ("Jacobi") form of UMAP's layout optimisation per launch.  Every
// vertex is updated from the snapshot of the previous epoch; every contribution is rounded to a multiple of 2^-32 and
// added as an int64, so a row's sum does not depend on the order and the layout is a pure function of the arguments
// (tests/_umap_oracle.py restates the rules).  The library is built -ffp-contract=off: the float64 expressions below
// are evaluated as written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icv_graph.hpp"  // ld_mix, ld_wave_sum, kGraphLongRow, k_graph_check (rule 1)

namespace icv {

constexpr int kUmLdsRow = kGraphLongRow; // longest row a wavefront stages; longer rows take a workgroup
constexpr int kUmMaxNegatives = 64;   // negative_sample_rate <= this

struct UmEpoch {
    double a, b;
    double c_att;   // (-2 a) b
    double c_rep;   // (2 gamma) b
    double alpha;   // initial_alpha (1 - t / n_epochs)
    double w_max;   // largest stored weight
    double w_min;   // w_max / n_epochs: lighter entries never fire
    double t, tm1;  // the epoch and the one before it
    uint64_t base;  // mix(seed ^ mix(t))
    int64_t n;
    int r;          // negative_sample_rate
};

// ---- rule 2: is the entry of weight w active in epoch t (t >= 1)? ------------------------------------------------------
__device__ __forceinline__ bool um_active(float wf, const UmEpoch& P) {
    const double w = (double)wf;
    if (!(w > 0.0) || w < P.w_min) return false;
    const double p = P.w_max / w;
    return floor(P.t / p) > floor(P.tm1 / p);
}

// ---- rules 3-5: contribution s of entry `ent` of row i (s = 0: the edge itself; s = 1 .. r: negative sample s - 1) ----
template <int C>
__device__ __forceinline__ void um_contribution(const float* __restrict__ y, const int32_t* __restrict__ col,
                                                const double (&yi)[C], int64_t i, int64_t ent, int s, const UmEpoch& P,
                                                long long (&acc)[C]) {
    int64_t j;
    if (s == 0) {
        j = col[ent];
    } else {
        const uint64_t h = ld_mix(P.base ^ ((uint64_t)ent * (uint64_t)P.r + (uint64_t)(s - 1)));
        j = (int64_t)(((h >> 32) * (uint64_t)P.n) >> 32);
    }
    double d[C];
    double d2 = 0.0;
#pragma unroll
    for (int q = 0; q < C; ++q) {
        d[q] = yi[q] - (double)y[j * C + q];
        d2 = q == 0 ? d[q] * d[q] : d2 + d[q] * d[q];
    }
    if (!(d2 > 0.0) || (s != 0 && j == i)) return;
    const double pb = pow(d2, P.b);
    const double den = P.a * pb + 1.0;
    const double coef = s == 0 ? (P.c_att * (pb / d2)) / den : P.c_rep / ((0.001 + d2) * den);
#pragma unroll
    for (int q = 0; q < C; ++q) {
        double g = coef * d[q];
        g = g < -4.0 ? -4.0 : (g > 4.0 ? 4.0 : g);
        if (s == 0) g = 2.0 * g;
        acc[q] += __double2ll_rn(g * 4294967296.0);
    }
}

// rule 6
__device__ __forceinline__ float um_step(double yi, long long S, double alpha) {
    return (float)(yi + alpha * ((double)S * (1.0 / 4294967296.0)));
}

// One epoch.  Blocks [0, short_blocks): a wavefront per row, 4 rows per block.  The lanes first compact the row's
// active entries into LDS (no position is gathered for the others), then run over (active entry, 1 + r contributions).
// Blocks from short_blocks on: a workgroup per row of long_list, the threads over (entry, contribution).
// A row without an active entry copies its position.
template <int C>
__global__ __launch_bounds__(256) void k_um_epoch(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                  const float* __restrict__ val, const float* __restrict__ y,
                                                  float* __restrict__ out, const int32_t* __restrict__ long_list,
                                                  unsigned short_blocks, UmEpoch P) {
    __shared__ unsigned short s_e[4][kUmLdsRow];
    __shared__ long long s_acc[4][C];
    __shared__ int s_cnt[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per = 1 + P.r;
    long long acc[C];
#pragma unroll
    for (int q = 0; q < C; ++q) acc[q] = 0;

    if (blockIdx.x >= short_blocks) {  // ---- a long row
        const int64_t v = long_list[blockIdx.x - short_blocks];
        const int64_t b = indptr[v];
        const int64_t items = (indptr[v + 1] - b) * per;
        double yi[C];
#pragma unroll
        for (int q = 0; q < C; ++q) yi[q] = (double)y[v * C + q];
        int cnt = 0;
        for (int64_t it = threadIdx.x; it < items; it += 256) {
            const int64_t ent = b + it / per;
            if (!um_active(val[ent], P)) continue;
            ++cnt;
            um_contribution<C>(y, col, yi, v, ent, (int)(it % per), P, acc);
        }
#pragma unroll
        for (int q = 0; q < C; ++q) acc[q] = ld_wave_sum(acc[q]);
        cnt = __any(cnt) ? 1 : 0;
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < C; ++q) s_acc[wave][q] = acc[q];
            s_cnt[wave] = cnt;
        }
        __syncthreads();
        if (threadIdx.x < C) {
            const int q = threadIdx.x;
            const long long S = s_acc[0][q] + s_acc[1][q] + s_acc[2][q] + s_acc[3][q];
            const bool any = s_cnt[0] | s_cnt[1] | s_cnt[2] | s_cnt[3];
            const float old = y[v * C + q];
            out[v * C + q] = any ? um_step((double)old, S, P.alpha) : old;
        }
        return;
    }

    // ---- a short row per wavefront
    const int64_t v = (int64_t)blockIdx.x * 4 + wave;
    int64_t b = 0;
    int deg = -1;  // -1: not this wavefront's row
    if (v < P.n) {
        b = indptr[v];
        const int64_t d = indptr[v + 1] - b;
        if (d <= kUmLdsRow) deg = (int)d;
    }
    int na = 0;
    for (int i0 = 0; i0 < deg; i0 += 64) {
        const int i = i0 + lane;
        const bool act = i < deg && um_active(val[b + i], P);
        const unsigned long long m = __ballot(act);
        if (act) s_e[wave][na + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)i;
        na += __popcll(m);
    }
    __syncthreads();
    if (deg < 0) return;
    if (na == 0) {
        if (lane < C) out[v * C + lane] = y[v * C + lane];
        return;
    }
    double yi[C];
#pragma unroll
    for (int q = 0; q < C; ++q) yi[q] = (double)y[v * C + q];
    const int items = na * per;
    for (int it = lane; it < items; it += 64)
        um_contribution<C>(y, col, yi, v, b + s_e[wave][it / per], it % per, P, acc);
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const long long S = ld_wave_sum(acc[q]);
        if (lane == q) out[v * C + q] = um_step(yi[q], S, P.alpha);
    }
}

}  // namespace icv

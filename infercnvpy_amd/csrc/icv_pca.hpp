// tl.pca (reference src/infercnvpy/tl/__init__.py:33-75, scanpy's pp.pca with svd_solver="arpack"): the two passes
// over X_cnv.  Everything between them (the W x W eigenproblem, the sign rule) is host code in tl/_pca.py.
//
//   k_pca_panel_csr / k_pca_panel_dense   rows of the input -> dense row-major panel (float32 or float64) whose row
//                                         count is padded to kPcaKC with zero rows
//   k_gram_f64     upper-triangle 64 x 64 tiles of panel^T panel, float64 MFMA (v_mfma_f64_16x16x4_f64); one
//                  workgroup per (tile, block of kPcaKB cells): split-K over the cells, one partial tile per block
//   k_gram_reduce  G[i][j] = G[j][i] = ((G_old + P_0) + P_1) + ...: the partials of the blocks in cell order, no
//                  atomics; bitwise symmetric, and the same bits whatever the panel size as long as panels start on
//                  block boundaries (the caller's contract, icv_gram_f64 in include/infercnv_hip.h)
//   k_csr_project / k_dense_project       X_pca = X V (- shift): one wavefront per row, lanes over components,
//                                         float64 sums in stored-entry order, float32 or float64 output
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace icv {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kPcaT = 64;      // output tile edge
constexpr int kPcaKC = 32;     // cells per LDS stage
constexpr int kPcaKB = 8192;   // cells per split-K block (one partial tile each); a multiple of kPcaKC
constexpr int kPcaLds = 66;    // LDS row stride in doubles (16-byte aligned rows, the 4 row groups of a read on
                               // different banks)

// panel[q][c] = X[q][c] for q < n_rows, 0 for the padding rows up to a multiple of kPcaKC; the panel was zeroed by the
// caller, CSR rows only scatter their stored entries (one wavefront per row).  indptr: absolute offsets of the rows.
template <typename T, typename P>
__global__ void __launch_bounds__(256) k_pca_panel_csr(const T* __restrict__ data, const int64_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ indices, int64_t n_rows,
                                                       P* __restrict__ panel, int64_t ldp) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_rows) return;
    P* o = panel + q * ldp;
    const int64_t e1 = indptr[q + 1];
    for (int64_t k = indptr[q] + (threadIdx.x & 63); k < e1; k += 64) o[indices[k]] = (P)data[k];
}

template <typename T, typename P>
__global__ void __launch_bounds__(256) k_pca_panel_dense(const T* __restrict__ x, int64_t ld, int64_t n_rows,
                                                         int n_cols, P* __restrict__ panel, int64_t ldp) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_rows) return;
    const T* xr = x + q * ld;
    P* o = panel + q * ldp;
    for (int c = threadIdx.x & 63; c < n_cols; c += 64) o[c] = (P)xr[c];
}

// Workgroup = 4 wavefronts in 2 x 2, each a 32 x 32 quadrant of the 64 x 64 tile (bi, bj), bi <= bj, as 2 x 2 MFMA
// tiles of 16 x 16.  v_mfma_f64_16x16x4_f64 (cdna_hip_programming.md, fragment layout): lane l holds A[i = l & 15]
// [k = l >> 4] and B[k = l >> 4][j = l & 15]; D register r is row (l >> 4) + 4 r, column l & 15.  A = the panel's
// columns of block bi (transposed: the sum runs over cells), B = those of block bj, so both operands are the same
// lane pattern on the LDS image of a stage (rows = cells).  The next stage's global loads are in registers while
// the current one is multiplied.  Panel columns past n_cols only reach output elements the reduction skips.
//
// Grid: x = triangle tile (row-major over bi <= bj), y = block of kPcaKB cells of the panel.  The panel has
// n_pad = n_rows rounded up to kPcaKC rows.  Partial tile (block, tile) at part + (block * n_tri + tile) * 4096.
template <typename P>
__global__ void __launch_bounds__(256) k_gram_f64(const P* __restrict__ panel, int64_t ldp, int64_t n_pad, int n_t,
                                                  double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double sa[kPcaKC * kPcaLds];
    __shared__ __attribute__((aligned(16))) double sb[kPcaKC * kPcaLds];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_tri = n_t * (n_t + 1) / 2;
    int bi = 0, rem = (int)blockIdx.x;
    while (rem >= n_t - bi) rem -= n_t - bi, ++bi;
    const int bj = bi + rem;
    const int64_t c0 = (int64_t)blockIdx.y * kPcaKB;
    const int64_t c1 = c0 + kPcaKB < n_pad ? c0 + kPcaKB : n_pad;  // n_pad and kPcaKB are multiples of kPcaKC
    const P* pa = panel + (int64_t)bi * kPcaT;
    const P* pb = panel + (int64_t)bj * kPcaT;
    // stage loader: element e = t + 256 u (u < 8) is (row e >> 6, column e & 63): 64 consecutive values per row
    double ra[8], rb[8];
    auto load = [&](int64_t cs) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = t + 256 * u;
            const int64_t off = (cs + (e >> 6)) * ldp + (e & 63);
            ra[u] = (double)pa[off];
            rb[u] = (double)pb[off];
        }
    };
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const int lr = lane >> 4, lc = lane & 15;
    load(c0);
    for (int64_t cs = c0; cs < c1; cs += kPcaKC) {
        __syncthreads();  // the previous stage's reads are done
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = t + 256 * u;
            sa[(e >> 6) * kPcaLds + (e & 63)] = ra[u];
            sb[(e >> 6) * kPcaLds + (e & 63)] = rb[u];
        }
        __syncthreads();
        if (cs + kPcaKC < c1) load(cs + kPcaKC);
#pragma unroll
        for (int s = 0; s < kPcaKC / 4; ++s) {
            const int r = (4 * s + lr) * kPcaLds;
            const double a0 = sa[r + wi + lc], a1 = sa[r + wi + 16 + lc];
            const double b0 = sb[r + wj + lc], b1 = sb[r + wj + 16 + lc];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double* pt = part + ((int64_t)blockIdx.y * n_tri + blockIdx.x) * (kPcaT * kPcaT);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                pt[(wi + 16 * a + lr + 4 * r) * kPcaT + wj + 16 * b + lc] = acc[a][b][r];
}

// One workgroup per triangle tile, 16 elements per thread.  On a diagonal tile only i <= j is read; both mirror
// positions get the same value.  accumulate = 0: the sum starts from +0.0 instead of G's old value.
__global__ void __launch_bounds__(256) k_gram_reduce(const double* __restrict__ part, int n_blocks, int n_t, int n,
                                                     double* __restrict__ g, int64_t ldg, int accumulate) {
    const int n_tri = n_t * (n_t + 1) / 2;
    int bi = 0, rem = (int)blockIdx.x;
    while (rem >= n_t - bi) rem -= n_t - bi, ++bi;
    const int bj = bi + rem;
    for (int e = threadIdx.x; e < kPcaT * kPcaT; e += 256) {
        const int i = e >> 6, j = e & 63;
        const int gi = bi * kPcaT + i, gj = bj * kPcaT + j;
        if (gi >= n || gj >= n || (bi == bj && i > j)) continue;
        double s = accumulate ? g[(int64_t)gi * ldg + gj] : 0.0;
        for (int b = 0; b < n_blocks; ++b) s += part[((int64_t)b * n_tri + blockIdx.x) * (kPcaT * kPcaT) + e];
        g[(int64_t)gi * ldg + gj] = s;
        g[(int64_t)gj * ldg + gi] = s;
    }
}

// out[q][c] = sum over the stored entries of row q, in stored order, of x * v[col][c] (float64 fma chain), minus
// shift[c] when shift is given.  v: n_cols x k row-major float64.  One wavefront per row, lane c, c + 64, ...
template <typename T, typename O>
__global__ void __launch_bounds__(256) k_csr_project(const T* __restrict__ data, const int64_t* __restrict__ indptr,
                                                     const int32_t* __restrict__ indices, int64_t n_rows,
                                                     const double* __restrict__ v, int k,
                                                     const double* __restrict__ shift, O* __restrict__ out,
                                                     int64_t ldo) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t e0 = indptr[q], e1 = indptr[q + 1];
    for (int c = lane; c < k; c += 64) {
        double s = 0.0;
        for (int64_t e = e0; e < e1; ++e) s = fma((double)data[e], v[(int64_t)indices[e] * k + c], s);
        if (shift) s -= shift[c];
        out[q * ldo + c] = (O)s;
    }
}

// Dense counterpart: zero elements are skipped, so a dense row gives the bits of the same row stored as CSR.
template <typename T, typename O>
__global__ void __launch_bounds__(256) k_dense_project(const T* __restrict__ x, int64_t ld, int64_t n_rows, int n_cols,
                                                       const double* __restrict__ v, int k,
                                                       const double* __restrict__ shift, O* __restrict__ out,
                                                       int64_t ldo) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const T* xr = x + q * ld;
    for (int c = lane; c < k; c += 64) {
        double s = 0.0;
        for (int j = 0; j < n_cols; ++j) {
            const double xv = (double)xr[j];
            if (xv != 0.0) s = fma(xv, v[(int64_t)j * k + c], s);
        }
        if (shift) s -= shift[c];
        out[q * ldo + c] = (O)s;
    }
}

}  // namespace icv

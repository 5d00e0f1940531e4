// The float64 moment and triangular-product core of the covariance detectors: Mahalanobis / MCD (outlier_maha.hip), the
// Gaussian mixtures (outlier_gmm.hip) and, for the weighted projection at the end, PCA and kernel PCA (outlier_pca.hip,
// outlier_kpca.hip).  "Every published bit is the same from run to run and for every workspace" holds because each sum
// below is written once and has one order.
//
//   rows     a row-weight policy says how a row enters a moment sum.  SupportRows: a 0/1 support mask or none; a row outside
//            the support is a zero operand and no multiply is added.  WeightedRows: a responsibility r; the row enters the
//            sum as r x and the covariance as A = r (x - m), B = x - m.
//   sum      moment_sum_slab: a thread per feature adds the rows of a slab of kMomSlab rows in order (WeightedRows: one more
//            thread adds the weights themselves).
//   cov      moment_cov_tile: a workgroup per (lower-triangle 16 x 16 tile, slab), each wave 256 rows of the slab, four rows per
//            v_mfma_f64_16x16x4_f64, gathered through the feature table and centred on the fly (a row past n or past d_s is
//            a zero operand), the four waves added in order.
//   combine  slab_total: the slab partials in ascending order onto the total of the chunks before.  moment_chunks cuts the slabs
//            (and tiles) of a call to the workspace, so the workspace decides how many slabs a launch takes and never the
//            order of a sum.
//   product  tri_product_sqnorm: ||W (x - mu)||^2 for a workgroup's 64 rows, W lower triangular.  Y = Z W^T is formed 64
//            columns i at a time (four f64 accumulators a wave); for each such group K runs in staged slabs of kMomKC = 32
//            up to the group's diagonal: Z [64 rows, 32] (gathered, centred) and W [64, 32] go through LDS, zero filled past
//            d_s and the rows.  K blocks above the diagonal of a 16-wide tile and tiles wholly past d_s are skipped (a
//            skipped tile's accumulators stay +0.0, which is what the zero operands would have left).  Staging K slabs was
//            chosen over a narrower row tile: the LDS need (34 KB) does not grow with d_s, four workgroups fit a CU, and W
//            is read once per 64 rows instead of once per 16.  Y is squared and summed in the registers.  An element sees
//            k = 0, 1, 2, ... and then i = 0, 1, 2, ... in the same order wherever its row sits.
#pragma once
#include <algorithm>

#include "vgan_common.hpp"

namespace vgan {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kMomSlab = VGAN_MAHA_SLAB_ROWS;         // rows of a moment slab
constexpr int kMomT = 16;                             // tile edge of the f64 MFMA
constexpr int kMomBR = 64, kMomBI = 64, kMomKC = 32;  // staged product: rows, columns of Y and K per staged slab

// The policies.  live: does the row take part; term: what x adds to the sum; weight, left: the covariance's r and its A
// operand from z = x - m.  term spells its condition out on an int row on purpose: through live() the compiler selects
// instead of branching, and the two loads of a row (x, the support byte) then wait for each other.
struct SupportRows {
    const uint8_t* sup;  // nullptr: every row
    static constexpr bool kCounted = false;
    __device__ __forceinline__ bool live(long row) const { return !sup || sup[row]; }
    __device__ __forceinline__ double weight(long row) const { return 1.0; }  // never multiplied with
    __device__ __forceinline__ double left(double r, double z) const { return z; }
    __device__ __forceinline__ double term(int row, double v) const { return (!sup || sup[row]) ? v : 0.0; }
};

struct WeightedRows {
    const double* w;
    static constexpr bool kCounted = true;  // the sum of the weights is a moment too
    __device__ __forceinline__ bool live(long row) const { return true; }
    __device__ __forceinline__ double weight(long row) const { return w[row]; }
    __device__ __forceinline__ double left(double r, double z) const { return r * z; }
    __device__ __forceinline__ double term(int row, double v) const { return w[row] * v; }
};

// out[f] = the sum over the rows of the slab that starts at row r0 of the weighted x_f, rows in order, for the ds features at
// feat[f0 ..]; kCounted: *out_weight = the sum of the weights.  w starts at row r0 as well.
template <class Rows>
__device__ __forceinline__ void moment_sum_slab(const float* __restrict__ X, long ldx, int n, const int32_t* __restrict__ feat, int f0,
                                                int ds, long r0, Rows w, double* __restrict__ out, double* __restrict__ out_weight) {
    const int rows = (int)min((long)kMomSlab, (long)n - r0);
    for (int f = threadIdx.x; f < ds + (Rows::kCounted ? 1 : 0); f += kBlock) {
        double a = 0.0;
        if (f < ds) {
            const float* col = X + r0 * ldx + feat[f0 + f];
            for (int r = 0; r < rows; ++r) {
                const double v = (double)col[(long)r * ldx];
                a += w.term(r, v);
            }
            out[f] = a;
        } else if constexpr (Rows::kCounted) {
            for (int r = 0; r < rows; ++r) a += w.weight(r);
            *out_weight = a;
        }
    }
}

// part[16 x 16] = the sum over the rows of slab `slab` of A_a B_b for the features a of tile row ti and b of tile column tj;
// w starts at row 0
template <class Rows>
__device__ __forceinline__ void moment_cov_tile(const float* __restrict__ X, long ldx, int n, const int32_t* __restrict__ feat, int f0,
                                                int ds, int ti, int tj, Rows w, int slab, const double* __restrict__ mean,
                                                double* __restrict__ part) {
    __shared__ double red[kBlock / kWave][kMomT * kMomT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fa = ti * kMomT + (lane & 15), fb = tj * kMomT + (lane & 15);
    const bool va = fa < ds, vb = fb < ds;
    const int ca = va ? feat[f0 + fa] : 0, cb = vb ? feat[f0 + fb] : 0;
    const double ma = va ? mean[f0 + fa] : 0.0, mb = vb ? mean[f0 + fb] : 0.0;
    const long rbase = (long)slab * kMomSlab + (long)wave * (kMomSlab / 4);
    const long rend = min((long)n, rbase + kMomSlab / 4);
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (long r16 = rbase; r16 < rend; r16 += 16) {  // the same trip count for the whole wave; rows past rend are zero operands
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // the loads of sixteen rows are in flight before the first product needs one
            const long row = r16 + 4 * q + (lane >> 4);
            const bool ok = row < rend && w.live(row);
            const double r = ok ? w.weight(row) : 0.0;
            a[q] = (ok && va) ? w.left(r, (double)X[row * ldx + ca] - ma) : 0.0;
            b[q] = (ok && vb) ? (double)X[row * ldx + cb] - mb : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[q], acc, 0, 0, 0);
    }
    // f64 result layout: column = lane & 15, row = (lane >> 4) + 4 i
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][((lane >> 4) + 4 * i) * kMomT + (lane & 15)] = acc[i];
    __syncthreads();
    const int e = threadIdx.x;
    part[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// a + src[0] + src[stride] + ... : the nslabs slab partials in ascending order onto a, the total of the chunks before (or 0)
__device__ __forceinline__ double slab_total(double a, const double* __restrict__ src, int nslabs, long stride) {
    for (int q = 0; q < nslabs; ++q) a += src[(long)q * stride];
    return a;
}

// The two chunk loops of a moments call over a workspace of `cells` doubles.  sum(slab0, nslabs, first, last): the slab sums
// (sum_width doubles a slab) and their combine; cov(tile0, ntiles, slab0, nslabs, first, last): the tile partials (16 x 16
// doubles a tile and slab) and theirs.  first / last: the chunk holds slab 0 / the last slab.  A step returns VGAN_OK or ends
// the call with its code.
template <class SumStep, class CovStep>
inline int moment_chunks(int n, int64_t cells, int64_t sum_width, int n_tiles, SumStep sum, CovStep cov) {
    const int nslabs = (n + kMomSlab - 1) / kMomSlab;
    const int per_sum = (int)std::min<int64_t>(nslabs, cells / sum_width);
    for (int j0 = 0; j0 < nslabs; j0 += per_sum) {
        const int nj = std::min(per_sum, nslabs - j0);
        if (const int rc = sum(j0, nj, j0 == 0 ? 1 : 0, j0 + nj == nslabs ? 1 : 0)) return rc;
    }
    const int64_t tile_cells = kMomT * kMomT;
    const int per_tiles = (int)std::min<int64_t>(n_tiles, cells / tile_cells);
    const int per_cov = (int)std::min<int64_t>(std::min(nslabs, 65535), cells / (tile_cells * per_tiles));
    for (int t0 = 0; t0 < n_tiles; t0 += per_tiles) {
        const int nt = std::min(per_tiles, n_tiles - t0);
        for (int j0 = 0; j0 < nslabs; j0 += per_cov) {
            const int nj = std::min(per_cov, nslabs - j0);
            if (const int rc = cov(t0, nt, j0, nj, j0 == 0 ? 1 : 0, j0 + nj == nslabs ? 1 : 0)) return rc;
        }
    }
    return VGAN_OK;
}

// ||W (x - mu)||^2 of the row r0 + wave * 16 + (lane & 15) of Xq, valid in every lane: W [d, d] lower triangular, the d
// features at feat[f0 ..], mu at mean[f0 ..].  Every thread of the workgroup calls it.  34 KB of LDS.
__device__ __forceinline__ double tri_product_sqnorm(const float* __restrict__ Xq, long ldq, int rows, long r0,
                                                     const int32_t* __restrict__ feat, int f0, int d, const double* __restrict__ mean,
                                                     const double* __restrict__ W) {
    // a row stride of 34 doubles: the 32 lanes of a half-wave (16 rows x 2 k) read 32 different bank pairs
    __shared__ double zs[kMomBR][kMomKC + 2];  // centred rows [row][k]
    __shared__ double ws[kMomBI][kMomKC + 2];  // W [i][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = wave * kMomT + (lane & 15);
    double total = 0.0;
    for (int i0 = 0; i0 < d; i0 += kMomBI) {
        f64x4 acc[kMomBI / kMomT];
#pragma unroll
        for (int t = 0; t < kMomBI / kMomT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        const int kend = min(d, i0 + kMomBI);
        for (int k0 = 0; k0 < kend; k0 += kMomKC) {
            __syncthreads();  // the previous slab has been read
            for (int q = tid; q < kMomBR * kMomKC; q += kBlock) {
                const int rr = q / kMomKC, kk = q % kMomKC;
                const bool ok = r0 + rr < rows && k0 + kk < d;
                zs[rr][kk] = ok ? (double)Xq[(r0 + rr) * ldq + feat[f0 + k0 + kk]] - mean[f0 + k0 + kk] : 0.0;
            }
            for (int q = tid; q < kMomBI * kMomKC; q += kBlock) {
                const int ii = q / kMomKC, kk = q % kMomKC;
                const bool ok = i0 + ii < d && k0 + kk <= i0 + ii;
                ws[ii][kk] = ok ? W[(long)(i0 + ii) * d + k0 + kk] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < kMomBI / kMomT; ++t) {
                const int top = i0 + t * kMomT + kMomT - 1;  // the last column of the tile: K blocks past it are above the diagonal
                if (top - (kMomT - 1) >= d) break;           // the tile lies wholly past d_s (the same for the whole workgroup)
#pragma unroll
                for (int ks = 0; ks < kMomKC; ks += 4) {
                    if (k0 + ks > top) break;
                    const int kk = ks + (lane >> 4);
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ws[t * kMomT + (lane & 15)][kk], zs[slot][kk], acc[t], 0, 0, 0);
                }
            }
        }
        // result layout: column = lane & 15 (the data row), row = (lane >> 4) + 4 j (the column i of Y)
#pragma unroll
        for (int t = 0; t < kMomBI / kMomT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) total += acc[t][j] * acc[t][j];
    }
    total += __shfl_xor(total, 16, 64);
    total += __shfl_xor(total, 32, 64);
    return total;
}

// sum_j w_j y_j^2, y_j = sum_k V[j][k] z_k, of the row r0 + wave * 16 + (lane & 15), valid in every lane: the staging of
// tri_product_sqnorm with a full K range (V [d, d] is dense, row j a component), z(row, k) the operand of row < rows at k < d
// and the weights wt [d] of 64 components at a time in LDS.  A 16-row tile of V whose weights are all 0 issues no MFMA, a
// group of 64 without weight is not staged: which ones are skipped depends on wt alone.  A lane adds w_j y_j^2 over its
// components in ascending order (j = (lane >> 4) + 4 i of each tile, tiles ascending), then the four lane groups are added as
// (g + g^1) + (g^2 + g^3).  Every thread of the workgroup calls it (outlier_pca.hip, outlier_kpca.hip).  34 KB of LDS.
template <class Operand>
__device__ __forceinline__ double weighted_projection_sqnorm(int rows, long r0, int d, const double* __restrict__ V,
                                                             const double* __restrict__ wt, Operand&& z) {
    // a row stride of 34 doubles: the 32 lanes of a half-wave (16 rows x 2 k) read 32 different bank pairs
    __shared__ double zs[kMomBR][kMomKC + 2];  // operand rows [row][k]
    __shared__ double vs[kMomBI][kMomKC + 2];  // V [j][k]
    __shared__ double wl[kMomBI];              // the weights of the group
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double total = 0.0;
    for (int i0 = 0; i0 < d; i0 += kMomBI) {
        __syncthreads();  // the previous group's weights have been read
        if (tid < kMomBI) wl[tid] = i0 + tid < d ? wt[i0 + tid] : 0.0;
        __syncthreads();
        bool act[kMomBI / kMomT], any = false;
#pragma unroll
        for (int t = 0; t < kMomBI / kMomT; ++t) {
            act[t] = false;
            for (int q = 0; q < kMomT; ++q) act[t] |= wl[t * kMomT + q] != 0.0;
            any |= act[t];
        }
        if (!any) continue;  // the same in every thread: it depends on wt alone
        f64x4 acc[kMomBI / kMomT];
#pragma unroll
        for (int t = 0; t < kMomBI / kMomT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < d; k0 += kMomKC) {
            __syncthreads();  // the previous slab has been read
            for (int e = tid; e < kMomBR * kMomKC; e += kBlock) {
                const int rr = e / kMomKC, kk = e % kMomKC;
                const bool ok = r0 + rr < rows && k0 + kk < d;
                zs[rr][kk] = ok ? z(r0 + rr, k0 + kk) : 0.0;
            }
            for (int e = tid; e < kMomBI * kMomKC; e += kBlock) {
                const int ii = e / kMomKC, kk = e % kMomKC;
                const bool ok = i0 + ii < d && k0 + kk < d;
                vs[ii][kk] = ok ? V[(long)(i0 + ii) * d + k0 + kk] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < kMomBI / kMomT; ++t) {
                if (!act[t]) continue;
#pragma unroll
                for (int ks = 0; ks < kMomKC; ks += 4) {
                    const int kk = ks + (lane >> 4);
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[t * kMomT + (lane & 15)][kk], zs[wave * kMomT + (lane & 15)][kk], acc[t],
                                                                  0, 0, 0);
                }
            }
        }
        // result layout: column = lane & 15 (the data row), row = (lane >> 4) + 4 j (the component)
#pragma unroll
        for (int t = 0; t < kMomBI / kMomT; ++t) {
            if (!act[t]) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) total += wl[t * kMomT + (lane >> 4) + 4 * j] * (acc[t][j] * acc[t][j]);
        }
    }
    total += __shfl_xor(total, 16, 64);
    total += __shfl_xor(total, 32, 64);
    return total;
}

}  // namespace vgan

// Mahalanobis / MCD outlier scores over the subspaces: a float64 mean and covariance per subspace, its shrunk Cholesky
// factor inverted into W_s = L_s^-1, and score = ||W_s (x - mu_s)||^2.  n d_s^2 per subspace, nothing n x n.  All arithmetic
// is float64 on the float32 data; every sum has a fixed order and there is no float atomic, so every published bit is the
// same from run to run and for every workspace.  The contract is the header's and the SubspaceMahalanobis docstring.
//
//   moments  rows are cut into slabs of kMomSlab rows, by n alone; the sum, covariance-tile, combine and chunking core is
//            outlier_moments.hpp's with the support as the row policy (a row outside it is a zero operand).  The slab
//            partials go to the workspace and one thread per element adds them in ascending slab order, so the workspace
//            decides how many slabs a launch takes and never the order of a sum; the last combine divides by h_s.
//   factor   one workgroup per subspace: trace and sum of squares (fixed block reductions), the shrinkage alpha (given or
//            OAS), Sigma = (1 - alpha) C + alpha (tr C / d) I written over C, then a blocked right-looking Cholesky with
//            16-wide blocks: the diagonal block is factored in LDS, the panel below it by one thread per row (a 16-step
//            substitution against the LDS block), the trailing lower triangle tile by tile on the f64 MFMA (K = 16, four
//            instructions a tile, the waves taking tiles in turn).  The panel itself stays in global memory: at d_s = 1024
//            it is 1008 x 16 doubles = 126 KB, more than a workgroup's static LDS, and the one CU that runs this workgroup
//            holds it in its cache.  L is then inverted into W a thread per column (forward substitution, k ascending).
//   scores   a workgroup per (subspace, 64 rows), a wave 16 rows: outlier_moments.hpp's staged lower-triangular product
//            (34 KB of LDS whatever d_s, so four workgroups fit a CU); the float32 store is the only rounding below float64.
//   select   one workgroup per subspace: a four-pass radix select on order-preserving keys finds the key of rank h - 1 and
//            how many rows of that key are wanted; an ordered sweep then marks every smaller key and the first wanted rows of
//            the equal one in row order, and compares with the previous support.  Integer LDS atomics only.
#include <math.h>

#include "outlier_moments.hpp"

namespace vgan {

// part[slab, feature]: the sum of the supported rows of the slab, rows in order
__global__ __launch_bounds__(kBlock) void maha_sum_kernel(const float* __restrict__ X, long ldx, int n, const int32_t* __restrict__ feat,
                                                          const int32_t* __restrict__ feat_off, int first,
                                                          const uint8_t* __restrict__ support, long ld_sup, int slab0,
                                                          double* __restrict__ part, int total_dims) {
    const int s = first + blockIdx.y;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0, base = f0 - feat_off[first];
    const long r0 = (long)(slab0 + blockIdx.x) * kMomSlab;
    moment_sum_slab(X, ldx, n, feat, f0, ds, r0, SupportRows{support ? support + (long)s * ld_sup + r0 : nullptr},
                    part + (long)blockIdx.x * total_dims + base, nullptr);
}

// mean (+)= the slab partials in ascending order; the last call divides by h_s
__global__ __launch_bounds__(kBlock) void maha_mean_combine_kernel(const double* __restrict__ part, int nslabs, int total_dims,
                                                                   const int32_t* __restrict__ feat_off, int first,
                                                                   const int32_t* __restrict__ hcount, double* __restrict__ mean,
                                                                   int first_chunk, int last) {
    const int s = first + blockIdx.y;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0, base = f0 - feat_off[first];
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= ds) return;
    double a = slab_total(first_chunk ? 0.0 : mean[f0 + f], part + base + f, nslabs, total_dims);
    if (last) a /= (double)hcount[s];
    mean[f0 + f] = a;
}

// part[slab, tile, 16 x 16]: sum over the supported rows of the slab of z_a z_b for the tile's features
__global__ __launch_bounds__(kBlock) void maha_cov_kernel(const float* __restrict__ X, long ldx, int n, const int32_t* __restrict__ feat,
                                                          const int32_t* __restrict__ feat_off, const int32_t* __restrict__ tiles,
                                                          const uint8_t* __restrict__ support, long ld_sup, int slab0,
                                                          const double* __restrict__ mean, double* __restrict__ part) {
    const int32_t* tl = tiles + 3L * blockIdx.x;
    const int s = tl[0], f0 = feat_off[s];
    moment_cov_tile(X, ldx, n, feat, f0, feat_off[s + 1] - f0, tl[1], tl[2], SupportRows{support ? support + (long)s * ld_sup : nullptr},
                    slab0 + blockIdx.y, mean, part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (kMomT * kMomT));
}

// cov (+)= the slab partials in ascending order, lower triangle and its mirror; the last call divides by h_s
__global__ __launch_bounds__(kBlock) void maha_cov_combine_kernel(const double* __restrict__ part, int nslabs, const int32_t* __restrict__ tiles,
                                                                  const int32_t* __restrict__ feat_off, const int64_t* __restrict__ sq_off,
                                                                  const int32_t* __restrict__ hcount, double* __restrict__ cov,
                                                                  int first_chunk, int last) {
    const int32_t* tl = tiles + 3L * blockIdx.x;
    const int s = tl[0], e = threadIdx.x;
    const int ds = feat_off[s + 1] - feat_off[s];
    const int i = tl[1] * kMomT + e / kMomT, j = tl[2] * kMomT + e % kMomT;
    if (i >= ds || j >= ds || j > i) return;
    double* C = cov + sq_off[s];
    double a = slab_total(first_chunk ? 0.0 : C[(long)i * ds + j], part + (long)blockIdx.x * (kMomT * kMomT) + e, nslabs,
                          (long)gridDim.x * (kMomT * kMomT));
    if (last) a /= (double)hcount[s];
    C[(long)i * ds + j] = a;
    C[(long)j * ds + i] = a;
}

// status: bit 0 the subspace is constant on its support (this call), bit 1 a pivot failed (this call or an earlier one)
__global__ __launch_bounds__(kBlock) void maha_factor_kernel(double* cov, const int64_t* __restrict__ sq_off,
                                                             const int32_t* __restrict__ feat_off, int first,
                                                             const int32_t* __restrict__ hcount, double shrink, double* Lall, double* Wall,
                                                             double* __restrict__ alpha_out, int32_t* __restrict__ status) {
    __shared__ double red[kBlock / kWave];
    __shared__ double blk[kMomT][kMomT + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = first + blockIdx.x;
    const int d = feat_off[s + 1] - feat_off[s];
    const long dd = (long)d * d;
    double* C = cov + sq_off[s];
    double* L = Lall + sq_off[s];
    double* W = Wall + sq_off[s];

    double tr = 0.0, sq = 0.0;
    for (int i = tid; i < d; i += kBlock) tr += C[(long)i * d + i];
    for (long e = tid; e < dd; e += kBlock) {
        const double c = C[e];
        sq += c * c;
    }
    tr = block_sum_all(tr, red);
    sq = block_sum_all(sq, red);
    const double m = tr / (double)d;
    double alpha = shrink;
    if (shrink < 0.0) {  // OAS
        const double a = sq / ((double)d * (double)d), m2 = m * m;
        const double den = ((double)hcount[s] + 1.0) * (a - m2 / (double)d);
        alpha = den == 0.0 ? 1.0 : fmin((a + m2) / den, 1.0);
    }
    const bool constant = tr == 0.0;
    const double keep = 1.0 - alpha, ridge = alpha * m;
    for (long e = tid; e < dd; e += kBlock) {
        const int i = (int)(e / d), j = (int)(e % d);
        const double v = keep * C[e] + (i == j ? ridge : 0.0);
        C[e] = v;
        L[e] = (!constant && j <= i) ? v : 0.0;
        if (constant) W[e] = 0.0;
    }
    int sticky = 0;  // thread 0 alone reads and writes the status word
    if (tid == 0) {
        sticky = status[s] & 2;
        alpha_out[s] = alpha;
    }
    if (constant) {
        if (tid == 0) status[s] = sticky | 1;
        return;
    }
    __syncthreads();

    const int T = (d + kMomT - 1) / kMomT;
    const int r = tid >> 4, c = tid & 15;
    bool failed = false;
    for (int k0 = 0; k0 < d && !failed; k0 += kMomT) {
        const int nb = min(kMomT, d - k0);
        // the diagonal block, padded with the identity
        blk[r][c] = (r < nb && c < nb) ? L[(long)(k0 + r) * d + k0 + c] : (r == c ? 1.0 : 0.0);
        __syncthreads();
        for (int j = 0; j < kMomT; ++j) {
            const double p = blk[j][j];
            if (!(p > 0.0 && p < INFINITY)) {  // the same value in every thread
                failed = true;
                break;
            }
            __syncthreads();
            const double sp = sqrt(p);
            if (c == j && r >= j) blk[r][j] = r == j ? sp : blk[r][j] / sp;
            __syncthreads();
            if (c > j && r >= c) blk[r][c] -= blk[r][j] * blk[c][j];
            __syncthreads();
        }
        if (failed) break;
        if (r < nb && c < nb) L[(long)(k0 + r) * d + k0 + c] = c <= r ? blk[r][c] : 0.0;
        // the panel below the block: row i solves x L_kk^T = A[i, k0 : k0 + 16]
        for (int i = k0 + kMomT + tid; i < d; i += kBlock) {
            double* row = L + (long)i * d + k0;
            double x[kMomT];
#pragma unroll
            for (int q = 0; q < kMomT; ++q) x[q] = row[q];
#pragma unroll
            for (int q = 0; q < kMomT; ++q) {
                double v = x[q];
#pragma unroll
                for (int p = 0; p < q; ++p) v -= x[p] * blk[q][p];
                x[q] = v / blk[q][q];
            }
#pragma unroll
            for (int q = 0; q < kMomT; ++q) row[q] = x[q];
        }
        __syncthreads();  // the panel is visible to the workgroup
        // the trailing lower triangle, tile (ti, tj) with k0 / 16 < tj <= ti < T: A -= P_ti P_tj^T
        const int kb = k0 / kMomT, cnt = T - kb - 1, ntile = cnt * (cnt + 1) / 2;
        for (int q = wave; q < ntile; q += kBlock / kWave) {
            int a = (int)((sqrtf(8.f * (float)q + 1.f) - 1.f) * 0.5f);
            while ((a + 1) * (a + 2) / 2 <= q) ++a;
            while (a * (a + 1) / 2 > q) --a;
            const int ti = kb + 1 + a, tj = kb + 1 + q - a * (a + 1) / 2;
            const int ia = ti * kMomT + (lane & 15), ib = tj * kMomT + (lane & 15);
            f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < kMomT; ks += 4) {
                const int kk = k0 + ks + (lane >> 4);
                const double pa = ia < d ? L[(long)ia * d + kk] : 0.0;
                const double pb = ib < d ? L[(long)ib * d + kk] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, pb, acc, 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int i = ti * kMomT + (lane >> 4) + 4 * t, j = tj * kMomT + (lane & 15);
                if (i < d && j < d && j <= i) L[(long)i * d + j] -= acc[t];
            }
        }
        __syncthreads();
    }
    if (failed) {
        if (tid == 0) status[s] = 2;
        return;
    }
    // W = L^-1, a thread per column: w_jj = 1 / l_jj, w_ij = -(sum_{k = j}^{i - 1} l_ik w_kj) / l_ii
    for (int j = tid; j < d; j += kBlock) {
        for (int i = 0; i < j; ++i) W[(long)i * d + j] = 0.0;
        W[(long)j * d + j] = 1.0 / L[(long)j * d + j];
        for (int i = j + 1; i < d; ++i) {
            const double* li = L + (long)i * d;
            double a = 0.0;
            for (int k = j; k < i; ++k) a += li[k] * W[(long)k * d + j];
            W[(long)i * d + j] = -a / li[i];
        }
    }
    if (tid == 0) status[s] = sticky;
}

__global__ __launch_bounds__(kBlock) void maha_scores_kernel(const float* __restrict__ Xq, long ldq, int rows, const int32_t* __restrict__ feat,
                                                             const int32_t* __restrict__ feat_off, const int64_t* __restrict__ sq_off,
                                                             int first, const double* __restrict__ mean, const double* __restrict__ Wall,
                                                             float* __restrict__ score, long ld_score) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = first + blockIdx.y;
    const int f0 = feat_off[s], d = feat_off[s + 1] - f0;
    const long r0 = (long)blockIdx.x * kMomBR;
    const double total = tri_product_sqnorm(Xq, ldq, rows, r0, feat, f0, d, mean, Wall + sq_off[s]);
    const long row = r0 + wave * kMomT + (lane & 15);
    if (lane < 16 && row < rows) score[(long)s * ld_score + row] = (float)total;
}

__device__ __forceinline__ uint32_t maha_key(float v) {  // order-preserving, -0.0 as +0.0
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kBlock) void maha_select_kernel(const float* __restrict__ score, long ld, int n, const int32_t* __restrict__ hcount,
                                                             int first, uint8_t* support, long ld_sup, int32_t* __restrict__ changed) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh_prefix, sh_rank, sh_running, sh_any;
    __shared__ unsigned wcount[kBlock / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = first + blockIdx.x;
    const float* row = score + (long)s * ld;
    uint8_t* sup = support + (long)s * ld_sup;
    const int h = max(1, min(hcount[s], n));
    unsigned prefix = 0u, rank = (unsigned)(h - 1);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < n; i += kBlock) {
            const unsigned key = maha_key(row[i]);
            if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned below = 0u;
            int digit = 0;
            for (; digit < 255; ++digit) {
                if (rank < below + hist[digit]) break;
                below += hist[digit];
            }
            sh_prefix = prefix | ((unsigned)digit << shift);
            sh_rank = rank - below;
        }
        __syncthreads();
        prefix = sh_prefix;
        rank = sh_rank;
        __syncthreads();
    }
    // every key below `prefix`, and the first rank + 1 rows that hold it
    const unsigned take = rank + 1u;
    if (tid == 0) {
        sh_running = 0u;
        sh_any = 0u;
    }
    __syncthreads();
    unsigned differs = 0u;
    for (int base = 0; base < n; base += kBlock) {
        const int i = base + tid;
        const unsigned key = i < n ? maha_key(row[i]) : 0xFFFFFFFFu;
        const bool eq = i < n && key == prefix;
        const unsigned long long votes = __ballot(eq);
        if (lane == 0) wcount[wave] = (unsigned)__popcll(votes);
        __syncthreads();
        unsigned before = sh_running;
        for (int w = 0; w < wave; ++w) before += wcount[w];
        before += (unsigned)__popcll(votes & ((1ull << lane) - 1ull));
        if (i < n) {
            const uint8_t in = (key < prefix || (eq && before < take)) ? 1 : 0;
            differs |= (unsigned)(sup[i] != in);
            sup[i] = in;
        }
        __syncthreads();
        if (tid == 0) sh_running += (wcount[0] + wcount[1]) + (wcount[2] + wcount[3]);
        __syncthreads();
    }
    if (differs) atomicOr(&sh_any, 1u);
    __syncthreads();
    if (tid == 0) changed[s] = (int32_t)sh_any;
}

}  // namespace vgan

using namespace vgan;

static bool maha_range_ok(int first, int count) { return first >= 0 && count > 0 && count <= 65535; }

extern "C" int vgan_maha_moments(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off,
                                 const int64_t* sq_off, int first, int count, int total_dims, int max_dims, const int32_t* tiles,
                                 int n_tiles, const uint8_t* support, int64_t ld_support, const int32_t* hcount, double* mean,
                                 double* cov, void* workspace, int64_t workspace_bytes, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && feat && feat_off && sq_off && tiles && hcount && mean && cov && workspace);
    VGAN_CHECK_ARG(d > 0 && ldx >= d && n >= 2 && n <= VGAN_MAHA_MAX_ROWS && maha_range_ok(first, count));
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= VGAN_MAHA_MAX_DIMS && total_dims >= count && total_dims <= (int64_t)count * max_dims);
    VGAN_CHECK_ARG(n_tiles >= count && (!support || ld_support >= n));
    VGAN_CHECK_ARG(workspace_bytes >= 8 * (int64_t)total_dims && workspace_bytes >= 8 * kMomT * kMomT);
    const hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(workspace);
    const dim3 mgrid((max_dims + kBlock - 1) / kBlock, count);
    return moment_chunks(
        n, workspace_bytes / 8, total_dims, n_tiles,
        [&](int j0, int nj, int first_chunk, int last) {
            hipLaunchKernelGGL(maha_sum_kernel, dim3(nj, count), dim3(kBlock), 0, st, X, (long)ldx, n, feat, feat_off, first, support,
                               (long)ld_support, j0, part, total_dims);
            hipLaunchKernelGGL(maha_mean_combine_kernel, mgrid, dim3(kBlock), 0, st, part, nj, total_dims, feat_off, first, hcount, mean,
                               first_chunk, last);
            VGAN_CHECK_LAUNCH();
            return VGAN_OK;
        },
        [&](int t0, int nt, int j0, int nj, int first_chunk, int last) {
            hipLaunchKernelGGL(maha_cov_kernel, dim3(nt, nj), dim3(kBlock), 0, st, X, (long)ldx, n, feat, feat_off, tiles + 3L * t0, support,
                               (long)ld_support, j0, mean, part);
            hipLaunchKernelGGL(maha_cov_combine_kernel, dim3(nt), dim3(kBlock), 0, st, part, nj, tiles + 3L * t0, feat_off, sq_off, hcount, cov,
                               first_chunk, last);
            VGAN_CHECK_LAUNCH();
            return VGAN_OK;
        });
}

extern "C" int vgan_maha_factor(double* cov, const int64_t* sq_off, const int32_t* feat_off, int first, int count, int max_dims,
                                const int32_t* hcount, double shrinkage, double* L, double* W, double* alpha, int32_t* status,
                                vgan_stream_t stream) {
    VGAN_CHECK_ARG(cov && sq_off && feat_off && hcount && L && W && alpha && status && maha_range_ok(first, count));
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= VGAN_MAHA_MAX_DIMS);
    VGAN_CHECK_ARG(shrinkage == VGAN_MAHA_SHRINKAGE_OAS || (shrinkage >= 0.0 && shrinkage <= 1.0));
    hipLaunchKernelGGL(maha_factor_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, cov, sq_off, feat_off, first, hcount, shrinkage,
                       L, W, alpha, status);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_maha_scores(const float* Xq, int ldq, int rows, int d, const int32_t* feat, const int32_t* feat_off,
                                const int64_t* sq_off, int first, int count, int max_dims, const double* mean, const double* W,
                                float* score, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && feat && feat_off && sq_off && mean && W && score && maha_range_ok(first, count));
    VGAN_CHECK_ARG(d > 0 && ldq >= d && rows > 0 && rows <= VGAN_MAHA_MAX_ROWS && ld_score >= rows);
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= VGAN_MAHA_MAX_DIMS);
    const dim3 grid((rows + kMomBR - 1) / kMomBR, count);
    hipLaunchKernelGGL(maha_scores_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, Xq, (long)ldq, rows, feat, feat_off, sq_off, first, mean,
                       W, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_maha_select(const float* score, int64_t ld_score, int n, int first, int count, const int32_t* hcount,
                                uint8_t* support, int64_t ld_support, int32_t* changed, vgan_stream_t stream) {
    VGAN_CHECK_ARG(score && hcount && support && changed && maha_range_ok(first, count));
    VGAN_CHECK_ARG(n >= 1 && n <= VGAN_MAHA_MAX_ROWS && ld_score >= n && ld_support >= n);
    hipLaunchKernelGGL(maha_select_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, score, (long)ld_score, n, hcount, first, support,
                       (long)ld_support, changed);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

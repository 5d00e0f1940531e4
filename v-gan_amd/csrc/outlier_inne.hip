// iNNE (Bandaragoda, Ting, Albrecht, Liu, Wells 2018; pyod's INNE) over the subspaces: T estimators per subspace, each psi
// sampled rows (the centres) with a hypersphere around every centre that reaches its nearest other centre; a query row takes
// from each estimator the isolation ratio of the smallest sphere that covers it, or 1 where none does.  Nothing here is
// n x n: the build touches psi^2 pairs per estimator, scoring T psi pairs per (row, subspace).
//
//   d2       the squared distance of two rows over the features of the subspace in ascending order, float64: per feature the
//            difference, its square and the sum are three separately rounded operations (mul_rounded_free keeps the product
//            out of an fma), so that every comparison here is the one a plain numpy loop makes.
//   build    one workgroup per estimator.  The psi row indices (feistel_perm of the estimator's stream, in that order: the
//            position breaks ties) live in LDS.  A pass owns kBlock centres, one a thread, and walks the other centres in
//            tiles of kInTile with one float64 accumulator each in registers; the features of both sides come through LDS in
//            tiles of kInFeat (the pass's centres as float32 rows padded to kInFeat + 1 words, the tile's as float64 [feature]
//            [centre], read as a broadcast).  The feature tiles are the inner loop, so a pair's sum runs over the features in
//            ascending order whatever the tiling, and the psi x psi matrix is never stored.  After a tile the thread keeps the
//            smaller (d2, position); positions ascend, so a strict < does it.  r2 and nn stay in LDS for the ratio
//            rho_j = 1 - (r2[nn_j] + eps) / (r2_j + eps), eps = 2^-52 (square roots of r2 for the paper's ratio), then rows,
//            r2, nn and rho are stored once.  Loads: psi d_s per tile of kInTile centres and pass.
//   scores   the hot path.  A workgroup owns one subspace and kBlock query rows, one a thread.  The T psi centres of the
//            subspace form one list (estimator-major); a tile of kInTile of them is staged per feature tile as float64
//            [feature][centre] (converted once at staging: the conversion is exact and the inner loop then holds the three
//            float64 operations and no conversion), with their r2 and rho; the query rows' features come through LDS as
//            float32 rows, gathered from Xq as given, once per workgroup where the subspace fits one feature tile and per
//            centre tile otherwise.  A thread keeps kInTile float64 accumulators, then walks the tile in list order: a centre
//            with d2 <= r2 whose r2 is smaller than the best so far replaces it (strict <: the lower position wins ties), and
//            the last centre of an estimator adds the best rho, or 1.0, to the row's float64 total, so the total runs over t
//            ascending.  No atomics, nothing depends on the launch.  score = float32(total / double(T)).
#include "vgan_common.hpp"

namespace vgan {

constexpr int kInMaxSamples = VGAN_INNE_MAX_SAMPLES;  // psi
constexpr int kInMaxDims = VGAN_INNE_MAX_DIMS;        // features of one subspace
constexpr int kInTile = 16;                           // centres of one register tile: 32 VGPRs of accumulators
constexpr int kInFeat = 32;                           // features of one staged tile
constexpr int kInPad = kInFeat + 1;                   // words of a staged float32 row: lanes over rows hit 64 banks

// acc[c] += (x - centre c)^2 over the fw features of the staged tile, ascending; the tile's row of a feature is read whole
// before the first difference is taken
__device__ __forceinline__ void inne_accumulate(const float* __restrict__ mine, const double (*__restrict__ tile)[kInTile], int fw,
                                                double (&acc)[kInTile]) {
    for (int f = 0; f < fw; ++f) {
        const double a = (double)mine[f];
        double b[kInTile];
#pragma unroll
        for (int c = 0; c < kInTile; ++c) b[c] = tile[f][c];
#pragma unroll
        for (int c = 0; c < kInTile; ++c) {
            const double diff = a - b[c];
            acc[c] += mul_rounded_free(diff, diff);
        }
    }
}

__global__ __launch_bounds__(kBlock) void inne_build_kernel(const float* __restrict__ X, long ldx, unsigned long long n,
                                                            const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                            int first, int T, int psi, int distance_ratio, int w,
                                                            unsigned long long seed, int32_t* __restrict__ rows_out,
                                                            double* __restrict__ r2_out, int32_t* __restrict__ nn_out,
                                                            double* __restrict__ rho_out) {
    __shared__ int rows[kInMaxSamples];
    __shared__ int nns[kInMaxSamples];
    __shared__ double r2s[kInMaxSamples];
    __shared__ float xj[kBlock][kInPad];
    __shared__ __attribute__((aligned(16))) double xi[kInFeat][kInTile];
    const int tid = threadIdx.x;
    const int s = first + (int)(blockIdx.x / (unsigned)T), t = (int)(blockIdx.x % (unsigned)T);
    const unsigned long long id = (unsigned long long)s * (unsigned long long)T + (unsigned long long)t;
    const int off = feat_off[s], ds = min(feat_off[s + 1] - off, kInMaxDims);
    const int nft = (ds + kInFeat - 1) / kInFeat;

    for (int i = tid; i < psi; i += kBlock) rows[i] = (int)feistel_perm((unsigned long long)i, n, w, seed, id);
    __syncthreads();

    for (int jb = 0; jb < psi; jb += kBlock) {
        const int j = jb + tid;
        double best = INFINITY;
        int best_at = j == 0 ? 1 : 0;  // in range whatever the comparisons say (NaN input)
        for (int i0 = 0; i0 < psi; i0 += kInTile) {
            double acc[kInTile];
#pragma unroll
            for (int c = 0; c < kInTile; ++c) acc[c] = 0.0;
            for (int ft = 0; ft < nft; ++ft) {
                const int f0 = ft * kInFeat, fw = min(kInFeat, ds - f0);
                __syncthreads();  // the previous tiles have been read
                if (nft > 1 || i0 == 0)  // a single feature tile stays staged for the whole pass
                    for (int e = tid; e < kBlock * kInFeat; e += kBlock) {
                        const int c = e / kInFeat, f = e % kInFeat;
                        xj[c][f] = (jb + c < psi && f < fw) ? X[(long)rows[jb + c] * ldx + feat[off + f0 + f]] : 0.f;
                    }
                for (int e = tid; e < kInTile * kInFeat; e += kBlock) {
                    const int c = e / kInFeat, f = e % kInFeat;
                    xi[f][c] = (i0 + c < psi && f < fw) ? (double)X[(long)rows[i0 + c] * ldx + feat[off + f0 + f]] : 0.0;
                }
                __syncthreads();
                inne_accumulate(xj[tid], xi, fw, acc);
            }
#pragma unroll
            for (int c = 0; c < kInTile; ++c) {
                const int i = i0 + c;
                if (i < psi && i != j && acc[c] < best) {
                    best = acc[c];
                    best_at = i;
                }
            }
        }
        if (j < psi) {
            r2s[j] = best;
            nns[j] = best_at;
        }
    }
    __syncthreads();
    const long out = ((long)s * T + t) * psi;
    for (int j = tid; j < psi; j += kBlock) {
        const double eps = 0x1p-52;
        double mine = r2s[j], theirs = r2s[nns[j]];
        if (distance_ratio) {
            mine = sqrt(mine);
            theirs = sqrt(theirs);
        }
        rows_out[out + j] = rows[j];
        r2_out[out + j] = r2s[j];
        nn_out[out + j] = nns[j];
        rho_out[out + j] = 1.0 - (theirs + eps) / (mine + eps);
    }
}

__global__ __launch_bounds__(kBlock) void inne_scores_kernel(const float* __restrict__ Xq, long ldq, int nq, const float* __restrict__ X,
                                                             long ldx, int n, const int32_t* __restrict__ feat,
                                                             const int32_t* __restrict__ feat_off, int first, int T, int psi,
                                                             const int32_t* __restrict__ rows, const double* __restrict__ r2,
                                                             const double* __restrict__ rho, float* __restrict__ score, long ld_score) {
    __shared__ float xq[kBlock][kInPad];
    __shared__ __attribute__((aligned(16))) double xc[kInFeat][kInTile];
    __shared__ double tile_r2[kInTile], tile_rho[kInTile];
    const int tid = threadIdx.x;
    const int z = blockIdx.y, s = first + z;
    const int off = feat_off[s], ds = min(feat_off[s + 1] - off, kInMaxDims);
    const int nft = (ds + kInFeat - 1) / kInFeat;
    const int centres = T * psi;  // at most 2^20
    const long base = (long)s * centres;
    const long q0 = (long)blockIdx.x * kBlock;
    double total = 0.0, best_r2 = 0.0, best_rho = 0.0;
    bool covered = false;

    for (int g0 = 0; g0 < centres; g0 += kInTile) {
        double acc[kInTile];
#pragma unroll
        for (int c = 0; c < kInTile; ++c) acc[c] = 0.0;
        for (int ft = 0; ft < nft; ++ft) {
            const int f0 = ft * kInFeat, fw = min(kInFeat, ds - f0);
            __syncthreads();  // the previous tiles have been read
            if (nft > 1 || g0 == 0)  // a single feature tile stays staged for the whole workgroup
                for (int e = tid; e < kBlock * kInFeat; e += kBlock) {
                    const int r = e / kInFeat, f = e % kInFeat;
                    xq[r][f] = (q0 + r < nq && f < fw) ? Xq[(q0 + r) * ldq + feat[off + f0 + f]] : 0.f;
                }
            for (int e = tid; e < kInTile * kInFeat; e += kBlock) {
                const int c = e / kInFeat, f = e % kInFeat;
                double v = 0.0;
                if (g0 + c < centres && f < fw) {
                    const int row = min(max(rows[base + g0 + c], 0), n - 1);  // a row of X whatever the buffer holds
                    v = (double)X[(long)row * ldx + feat[off + f0 + f]];
                }
                xc[f][c] = v;
            }
            if (ft == 0 && tid < kInTile) {
                const bool in = g0 + tid < centres;
                tile_r2[tid] = in ? r2[base + g0 + tid] : 0.0;
                tile_rho[tid] = in ? rho[base + g0 + tid] : 0.0;
            }
            __syncthreads();
            inne_accumulate(xq[tid], xc, fw, acc);
        }
        const int j0 = g0 % psi;
#pragma unroll
        for (int c = 0; c < kInTile; ++c) {
            if (g0 + c < centres) {  // the same for the whole workgroup
                const double r = tile_r2[c];
                if (acc[c] <= r && (!covered || r < best_r2)) {
                    covered = true;
                    best_r2 = r;
                    best_rho = tile_rho[c];
                }
                if ((j0 + c) % psi == psi - 1) {  // the estimator's last centre
                    total += covered ? best_rho : 1.0;
                    covered = false;
                }
            }
        }
    }
    if (q0 + tid < nq) score[(long)z * ld_score + q0 + tid] = (float)(total / (double)T);
}

}  // namespace vgan

using namespace vgan;

static bool inne_shape_ok(int T, int psi) { return T >= 1 && T <= VGAN_INNE_MAX_ESTIMATORS && psi >= 2 && psi <= kInMaxSamples; }

extern "C" int vgan_inne_build(const float* X, int ldx, int64_t n, int d, const int32_t* feat, const int32_t* feat_off, int first,
                               int count, int max_dims, int T, int psi, int ratio, uint64_t seed, int32_t* rows, double* r2, int32_t* nn,
                               double* rho, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && feat && feat_off && rows && r2 && nn && rho && d > 0 && ldx >= d && n >= 2 && n <= 0x7FFFFFFFLL);
    VGAN_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 && max_dims <= kInMaxDims && max_dims <= d);
    VGAN_CHECK_ARG(inne_shape_ok(T, psi) && psi <= n && (ratio == VGAN_INNE_RATIO_SQUARED || ratio == VGAN_INNE_RATIO_DISTANCE));
    hipLaunchKernelGGL(inne_build_kernel, dim3((unsigned)(count * T)), dim3(kBlock), 0, (hipStream_t)stream, X, (long)ldx,
                       (unsigned long long)n, feat, feat_off, first, T, psi, ratio == VGAN_INNE_RATIO_DISTANCE ? 1 : 0,
                       feistel_half_bits((unsigned long long)n), (unsigned long long)seed, rows, r2, nn, rho);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_inne_scores(const float* Xq, int ldq, int nq, int d, const float* X, int ldx, int64_t n, const int32_t* feat,
                                const int32_t* feat_off, int first, int count, int max_dims, int T, int psi, const int32_t* rows,
                                const double* r2, const double* rho, float* score, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && X && feat && feat_off && rows && r2 && rho && score && d > 0 && ldq >= d && ldx >= d && nq > 0);
    VGAN_CHECK_ARG(n >= 2 && n <= 0x7FFFFFFFLL && first >= 0 && count > 0 && count <= 65535 && ld_score >= nq);
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= kInMaxDims && max_dims <= d && inne_shape_ok(T, psi) && psi <= n);
    hipLaunchKernelGGL(inne_scores_kernel, dim3((unsigned)(((long)nq + kBlock - 1) / kBlock), count), dim3(kBlock), 0, (hipStream_t)stream,
                       Xq, (long)ldq, nq, X, (long)ldx, (int)n, feat, feat_off, first, T, psi, rows, r2, rho, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

// Gaussian-mixture outlier scores over the subspaces: EM for C full-covariance components per subspace (sklearn's
// GaussianMixture, covariance_type "full"; pyod's GMM), score = -log sum_c w_c N(x; mu_c, Sigma_c).  All arithmetic is float64
// on the float32 data; every sum has a fixed order and there is no float atomic, so every published bit is the same from run
// to run, for every workspace and for a subspace fitted alone or beside others.  The contract is the header's and the
// SubspaceGMM docstring.
//
// The (subspace, component) pairs are the entries e = s C + c of an EXPANDED subspace table (the feature list of s repeated C
// times; feat_off, sq_off accordingly), so that vgan_maha_factor factors and inverts the C covariances of every subspace
// unchanged.  A subspace whose done flag is set is frozen: the workgroups of the moments and of the E step that belong to it
// return at once, and the factor re-emits its matrices from an unchanged covariance.
//
//   moments  the sum, covariance-tile, combine and chunking core of outlier_moments.hpp (which vgan_maha_moments runs on too)
//            with the responsibility as the row weight.  sum: r_ic x_i over the rows of a slab in order, one more thread adds
//            r_ic (nk); the slab partials are added in ascending order; a workgroup per subspace then forms nk + 10 eps, w, log w
//            and divides the means.  cov: A = r_ic (x_i - mu_c), B = (x_i - mu_c); the combine divides by nk and adds reg_covar
//            on the diagonal.
//   logdet   a workgroup per entry: sum_j log L[j, j] in a fixed order.
//   estep    a workgroup per (subspace, 64 rows), a wave 16 rows, loops over the C components.  A component is the staged
//            lower-triangular product of outlier_moments.hpp (vgan_maha_scores', the float64 d^2 never rounded); its log
//            probability goes to LDS [32][64].  The lane that owns a row then takes the maximum, the sum of exponentials (c
//            ascending) and ln_i, writes the responsibilities (as exp(lp - max) / sum) and / or float32(-ln_i), and the
//            workgroup writes the sum of its 64 ln_i (a fixed butterfly over the 16 rows of a wave, the four waves in order).
//   converge a workgroup per subspace: a thread adds the 16 workgroup sums of a slab of 1024 rows in order, thread 0 the slabs
//            in ascending order; lb = sum / n; then sklearn's rule |lb - lb_prev| < tol, the iteration count and the done flag.
#include <float.h>
#include <math.h>

#include "outlier_moments.hpp"

namespace vgan {

constexpr int kGmmMaxC = VGAN_GMM_MAX_COMPONENTS;
constexpr double kGmmLog2Pi = 1.8378770664093454835606594728112;
static_assert(kMomSlab % kMomBR == 0, "a slab is a whole number of E-step workgroups");

// part[slab, entry feature]: sum over the rows of the slab of r x, rows in order; part[slab, total_dims + entry]: sum of r
__global__ __launch_bounds__(kBlock) void gmm_sum_kernel(const float* __restrict__ X, long ldx, int n, const int32_t* __restrict__ feat,
                                                         const int32_t* __restrict__ feat_off, int first, int C,
                                                         const double* __restrict__ resp, const int32_t* __restrict__ done, int slab0,
                                                         double* __restrict__ part, int total_dims, int entries) {
    const int rel = blockIdx.y, e = first * C + rel;
    if (done && done[e / C]) return;
    const int f0 = feat_off[e], ds = feat_off[e + 1] - f0, base = f0 - feat_off[first * C];
    const long r0 = (long)(slab0 + blockIdx.x) * kMomSlab;
    double* out = part + (long)blockIdx.x * (total_dims + entries);
    moment_sum_slab(X, ldx, n, feat, f0, ds, r0, WeightedRows{resp + (long)rel * n + r0}, out + base, out + total_dims + rel);
}

// mean, nk (+)= the slab partials in ascending order (raw sums: gmm_weights_kernel finishes them)
__global__ __launch_bounds__(kBlock) void gmm_sum_combine_kernel(const double* __restrict__ part, int nslabs, int total_dims, int entries,
                                                                 const int32_t* __restrict__ feat_off, int first, int C,
                                                                 const int32_t* __restrict__ done, double* __restrict__ mean,
                                                                 double* __restrict__ nk, int first_chunk) {
    const int rel = blockIdx.y, e = first * C + rel;
    if (done && done[e / C]) return;
    const int f0 = feat_off[e], ds = feat_off[e + 1] - f0, base = f0 - feat_off[first * C];
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f > ds) return;
    double* dst = f < ds ? mean + f0 + f : nk + e;
    const double* src = part + (f < ds ? base + f : total_dims + rel);
    *dst = slab_total(first_chunk ? 0.0 : *dst, src, nslabs, total_dims + entries);
}

// per subspace: nk_c = sum + 10 eps, w_c = nk_c / sum_c nk_c (c ascending), log w_c, mu_c = sum / nk_c
__global__ __launch_bounds__(kBlock) void gmm_weights_kernel(const int32_t* __restrict__ feat_off, int first, int C,
                                                             const int32_t* __restrict__ done, double* __restrict__ mean,
                                                             double* __restrict__ nk, double* __restrict__ weights, double* __restrict__ logw) {
    __shared__ double nks[kGmmMaxC];
    const int s = first + blockIdx.x, tid = threadIdx.x;
    if (done && done[s]) return;
    if (tid < C) nks[tid] = nk[s * C + tid] + 10.0 * DBL_EPSILON;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int c = 0; c < C; ++c) tot += nks[c];
        for (int c = 0; c < C; ++c) {
            const double w = nks[c] / tot;
            nk[s * C + c] = nks[c];
            weights[s * C + c] = w;
            logw[s * C + c] = log(w);
        }
    }
    for (int c = 0; c < C; ++c) {
        const int f0 = feat_off[s * C + c], ds = feat_off[s * C + c + 1] - f0;
        const double k = nks[c];
        for (int f = tid; f < ds; f += kBlock) mean[f0 + f] /= k;
    }
}

// part[slab, tile, 16 x 16]: sum over the rows of the slab of r z_a z_b for the tile's features
__global__ __launch_bounds__(kBlock) void gmm_cov_kernel(const float* __restrict__ X, long ldx, int n, const int32_t* __restrict__ feat,
                                                         const int32_t* __restrict__ feat_off, const int32_t* __restrict__ tiles, int first,
                                                         int C, const double* __restrict__ resp, const int32_t* __restrict__ done, int slab0,
                                                         const double* __restrict__ mean, double* __restrict__ part) {
    const int32_t* tl = tiles + 3L * blockIdx.x;
    const int e = tl[0];
    if (done && done[e / C]) return;
    const int f0 = feat_off[e];
    moment_cov_tile(X, ldx, n, feat, f0, feat_off[e + 1] - f0, tl[1], tl[2], WeightedRows{resp + (long)(e - first * C) * n},
                    slab0 + blockIdx.y, mean, part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (kMomT * kMomT));
}

// cov (+)= the slab partials in ascending order, lower triangle and its mirror; the last call divides by nk and adds reg_covar
__global__ __launch_bounds__(kBlock) void gmm_cov_combine_kernel(const double* __restrict__ part, int nslabs, const int32_t* __restrict__ tiles,
                                                                 const int32_t* __restrict__ feat_off, const int64_t* __restrict__ sq_off,
                                                                 int C, const int32_t* __restrict__ done, const double* __restrict__ nk,
                                                                 double reg_covar, double* __restrict__ cov, int first_chunk, int last) {
    const int32_t* tl = tiles + 3L * blockIdx.x;
    const int e = tl[0], t = threadIdx.x;
    if (done && done[e / C]) return;
    const int ds = feat_off[e + 1] - feat_off[e];
    const int i = tl[1] * kMomT + t / kMomT, j = tl[2] * kMomT + t % kMomT;
    if (i >= ds || j >= ds || j > i) return;
    double* S = cov + sq_off[e];
    double a = slab_total(first_chunk ? 0.0 : S[(long)i * ds + j], part + (long)blockIdx.x * (kMomT * kMomT) + t, nslabs,
                          (long)gridDim.x * (kMomT * kMomT));
    if (last) {
        a /= nk[e];
        if (i == j) a += reg_covar;
    }
    S[(long)i * ds + j] = a;
    S[(long)j * ds + i] = a;
}

// logdet[e] = sum_j log L_e[j, j]: a thread takes j = tid, tid + 256, ..., then the fixed workgroup sum
__global__ __launch_bounds__(kBlock) void gmm_logdet_kernel(const double* __restrict__ Lall, const int32_t* __restrict__ feat_off,
                                                            const int64_t* __restrict__ sq_off, int first_entry, double* __restrict__ logdet) {
    __shared__ double red[kBlock / kWave];
    const int e = first_entry + blockIdx.x;
    const int d = feat_off[e + 1] - feat_off[e];
    const double* L = Lall + sq_off[e];
    double a = 0.0;
    for (int j = threadIdx.x; j < d; j += kBlock) a += log(L[(long)j * d + j]);
    a = block_sum(a, red);
    if (threadIdx.x == 0) logdet[e] = a;
}

__global__ __launch_bounds__(kBlock) void gmm_estep_kernel(const float* __restrict__ Xq, long ldq, int rows, const int32_t* __restrict__ feat,
                                                           const int32_t* __restrict__ feat_off, const int64_t* __restrict__ sq_off, int first,
                                                           int C, const double* __restrict__ mean, const double* __restrict__ Wall,
                                                           const double* __restrict__ logdet, const double* __restrict__ logw,
                                                           const int32_t* __restrict__ done, double* __restrict__ resp,
                                                           double* __restrict__ lbpart, int nblocks, float* __restrict__ score, long ld_score) {
    __shared__ double lps[kGmmMaxC][kMomBR];  // log w_c N(x_row; c): written and read by the lane that owns the row
    __shared__ double red[kBlock / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = first + blockIdx.y;
    if (done && done[s]) return;
    const long r0 = (long)blockIdx.x * kMomBR;
    const int slot = wave * kMomT + (lane & 15);
    for (int c = 0; c < C; ++c) {
        const int e = s * C + c;
        const int f0 = feat_off[e], d = feat_off[e + 1] - f0;
        const double total = tri_product_sqnorm(Xq, ldq, rows, r0, feat, f0, d, mean, Wall + sq_off[e]);
        if (lane < kMomT) lps[c][slot] = -0.5 * ((double)d * kGmmLog2Pi + total) - logdet[e] + logw[e];
    }
    double ln = 0.0;
    const long row = r0 + slot;
    if (lane < kMomT && row < rows) {
        double m = lps[0][slot];
        for (int c = 1; c < C; ++c) m = fmax(m, lps[c][slot]);
        double sum = 0.0;
        for (int c = 0; c < C; ++c) sum += exp(lps[c][slot] - m);
        ln = m + log(sum);
        if (resp)
            for (int c = 0; c < C; ++c)  // exp(lp - ln) as exp(lp - m) / sum: ln carries half an ulp of its own size, the quotient does not
                resp[((long)blockIdx.y * C + c) * rows + row] = exp(lps[c][slot] - m) / sum;
        if (score) score[(long)s * ld_score + row] = (float)(-ln);
    }
    if (lbpart) {  // the same for the whole workgroup
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) ln += __shfl_xor(ln, o, 64);
        if (lane == 0) red[wave] = ln;
        __syncthreads();
        if (tid == 0) lbpart[(long)blockIdx.y * nblocks + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// done: 0 running, VGAN_GMM_DONE_CONVERGED, VGAN_GMM_DONE_FAILED
__global__ __launch_bounds__(kBlock) void gmm_converge_kernel(double* __restrict__ lbpart, int nblocks, int n, int first, int C,
                                                              const int32_t* __restrict__ status, double tol, int it,
                                                              int32_t* __restrict__ done, int32_t* __restrict__ n_iter,
                                                              double* __restrict__ lower_bound, double* __restrict__ lb_prev) {
    const int s = first + blockIdx.x, tid = threadIdx.x;
    if (done[s]) return;  // the same for the whole workgroup: thread 0 writes it only after the last barrier
    constexpr int per = kMomSlab / kMomBR;
    double* part = lbpart + (long)blockIdx.x * nblocks;
    const int nslabs = (nblocks + per - 1) / per;
    if (it > 0) {
        for (int j = tid; j < nslabs; j += kBlock) {
            double a = 0.0;
            for (int q = j * per; q < min(nblocks, (j + 1) * per); ++q) a += part[q];
            part[j * per] = a;  // the slab's sum over its first workgroup's
        }
    }
    __syncthreads();
    if (tid != 0) return;
    int failed = 0;
    for (int c = 0; c < C; ++c) failed |= status[s * C + c];
    if (failed) {
        done[s] = VGAN_GMM_DONE_FAILED;
        return;
    }
    if (it == 0) return;
    double a = 0.0;
    for (int j = 0; j < nslabs; ++j) a += part[j * per];
    const double lb = a / (double)n;
    n_iter[s] = it;
    lower_bound[s] = lb;
    if (fabs(lb - lb_prev[s]) < tol)
        done[s] = VGAN_GMM_DONE_CONVERGED;
    else
        lb_prev[s] = lb;
}

}  // namespace vgan

using namespace vgan;

// count subspaces of C components: the entries of one launch are a grid dimension
static bool gmm_range_ok(int first, int count, int C) {
    return C >= 1 && C <= kGmmMaxC && first >= 0 && count > 0 && (int64_t)count * C <= 65535 && ((int64_t)first + count) * C <= INT32_MAX;
}

extern "C" int vgan_gmm_moments(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off,
                                const int64_t* sq_off, int n_components, int first, int count, int total_dims, int max_dims,
                                const int32_t* tiles, int n_tiles, const double* resp, const int32_t* done, double reg_covar,
                                double* nk, double* weights, double* log_weights, double* mean, double* cov, void* workspace,
                                int64_t workspace_bytes, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && feat && feat_off && sq_off && tiles && resp && nk && weights && log_weights && mean && cov && workspace);
    VGAN_CHECK_ARG(gmm_range_ok(first, count, n_components));
    VGAN_CHECK_ARG(d > 0 && ldx >= d && n >= 2 && n <= VGAN_MAHA_MAX_ROWS && reg_covar >= 0.0 && reg_covar < INFINITY);
    const int C = n_components, entries = count * C;
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= VGAN_MAHA_MAX_DIMS && total_dims >= entries && total_dims <= (int64_t)entries * max_dims);
    VGAN_CHECK_ARG(n_tiles >= entries);
    VGAN_CHECK_ARG(workspace_bytes >= 8 * ((int64_t)total_dims + entries) && workspace_bytes >= 8 * kMomT * kMomT);
    const hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(workspace);
    const dim3 mgrid((max_dims + 1 + kBlock - 1) / kBlock, entries);
    return moment_chunks(
        n, workspace_bytes / 8, (int64_t)total_dims + entries, n_tiles,
        [&](int j0, int nj, int first_chunk, int last) {
            hipLaunchKernelGGL(gmm_sum_kernel, dim3(nj, entries), dim3(kBlock), 0, st, X, (long)ldx, n, feat, feat_off, first, C, resp, done, j0,
                               part, total_dims, entries);
            hipLaunchKernelGGL(gmm_sum_combine_kernel, mgrid, dim3(kBlock), 0, st, part, nj, total_dims, entries, feat_off, first, C, done, mean,
                               nk, first_chunk);
            VGAN_CHECK_LAUNCH();
            if (last) {  // the sums are whole: nk, the weights and the means
                hipLaunchKernelGGL(gmm_weights_kernel, dim3(count), dim3(kBlock), 0, st, feat_off, first, C, done, mean, nk, weights, log_weights);
                VGAN_CHECK_LAUNCH();
            }
            return VGAN_OK;
        },
        [&](int t0, int nt, int j0, int nj, int first_chunk, int last) {
            hipLaunchKernelGGL(gmm_cov_kernel, dim3(nt, nj), dim3(kBlock), 0, st, X, (long)ldx, n, feat, feat_off, tiles + 3L * t0, first, C, resp,
                               done, j0, mean, part);
            hipLaunchKernelGGL(gmm_cov_combine_kernel, dim3(nt), dim3(kBlock), 0, st, part, nj, tiles + 3L * t0, feat_off, sq_off, C, done, nk,
                               reg_covar, cov, first_chunk, last);
            VGAN_CHECK_LAUNCH();
            return VGAN_OK;
        });
}

extern "C" int vgan_gmm_logdet(const double* L, const int32_t* feat_off, const int64_t* sq_off, int n_components, int first, int count,
                               double* logdet, vgan_stream_t stream) {
    VGAN_CHECK_ARG(L && feat_off && sq_off && logdet && gmm_range_ok(first, count, n_components));
    hipLaunchKernelGGL(gmm_logdet_kernel, dim3(count * n_components), dim3(kBlock), 0, (hipStream_t)stream, L, feat_off, sq_off,
                       first * n_components, logdet);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_gmm_estep(const float* Xq, int ldq, int rows, int d, const int32_t* feat, const int32_t* feat_off,
                              const int64_t* sq_off, int n_components, int first, int count, int max_dims, const double* mean,
                              const double* W, const double* logdet, const double* log_weights, const int32_t* done, double* resp,
                              double* lb_partial, float* score, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && feat && feat_off && sq_off && mean && W && logdet && log_weights && gmm_range_ok(first, count, n_components));
    VGAN_CHECK_ARG((resp || score) && (!score || ld_score >= rows) && (!lb_partial || resp));
    VGAN_CHECK_ARG(d > 0 && ldq >= d && rows > 0 && rows <= VGAN_MAHA_MAX_ROWS);
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= VGAN_MAHA_MAX_DIMS);
    const int nblocks = (rows + kMomBR - 1) / kMomBR;
    hipLaunchKernelGGL(gmm_estep_kernel, dim3(nblocks, count), dim3(kBlock), 0, (hipStream_t)stream, Xq, (long)ldq, rows, feat, feat_off, sq_off,
                       first, n_components, mean, W, logdet, log_weights, done, resp, lb_partial, nblocks, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_gmm_converge(double* lb_partial, int n, int n_components, int first, int count, const int32_t* status, double tol,
                                 int iteration, int32_t* done, int32_t* n_iter, double* lower_bound, double* lb_prev,
                                 vgan_stream_t stream) {
    VGAN_CHECK_ARG(status && done && n_iter && lower_bound && lb_prev && gmm_range_ok(first, count, n_components));
    VGAN_CHECK_ARG(n >= 2 && n <= VGAN_MAHA_MAX_ROWS && tol >= 0.0 && iteration >= 0 && (iteration == 0 || lb_partial));
    hipLaunchKernelGGL(gmm_converge_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, lb_partial, (n + kMomBR - 1) / kMomBR, n, first,
                       n_components, status, tol, iteration, done, n_iter, lower_bound, lb_prev);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

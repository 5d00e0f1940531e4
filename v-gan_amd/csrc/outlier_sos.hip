// Stochastic outlier selection over the subspaces (Janssens, Huszar, Postma, van den Herik 2012; pyod's SOS; the perplexity
// search of t-SNE; v-gan_amd/outlier.py: SubspaceSOS, whose docstring is the contract).
//
// Per subspace s:
//   1. matrix  outlier_dist.hpp's pair_matrix_kernel (both engines) over the packed block against itself, stored by reference
//              row: sqrtf(d2) or d2 itself.  Row i of D holds the dissimilarities of fitted row i (as the reference side) to all rows.
//   2. fit     per fitted row the root search for beta_i: the row's entries are read once and stay in LDS for all steps; a step
//              is a float64 exp per entry and two sums over the row.  A short row belongs to one wave (four rows per
//              workgroup, the sums are butterflies, no barrier), a long one to a workgroup of 1024 threads (a wave butterfly, one
//              LDS slot per wave, one barrier per step).  The sums are the same bits in every lane, so the stop is uniform.
//   3. scores  a row's terms min(-log1p(-b), 128) or min(log1p(a / Z), 128) are summed as rint(term 2^40) in 64-bit fixed point,
//              so the sum has no order: at fit from the stored matrix (a wave per scored row), for new rows through
//              outlier_dist.hpp's fixed_point_row_sums with the fitted rows as reference side, then exp(-sum).
#include <float.h>
#include <limits.h>

#include "outlier_dist.hpp"

namespace vgan {

constexpr int kSosWide = 1024;  // threads of the workgroup that owns a long row

__device__ __forceinline__ float sos_entry(int metric, float d2) { return metric == VGAN_SOS_METRIC_EUCLIDEAN ? sqrtf(d2) : d2; }

// pair_matrix_kernel's entry: the dissimilarity of query row q to reference row c, the same rule in every subspace
struct SosEntry {
    int metric;
    __device__ __forceinline__ SosEntry of(int) const { return *this; }
    __device__ __forceinline__ float operator()(int, int, float d2) const { return sos_entry(metric, d2); }
};

// The sums and the minimum of a row's owner, the same bits in every thread of it.  NT = 64: the owner is a wave, the xor
// butterfly leaves every lane with the same value (each level adds the same two numbers in either lane).  NT = 1024: lane 0 of
// every wave writes the wave's value to its slot, and after the barrier every thread adds the slots in order.  The callers
// alternate between two slot sets, so that one barrier per use is enough.
template <int NT>
__device__ __forceinline__ void sos_sum2(double& a, double& b, double* slots) {
    a = wave_sum(a);
    b = wave_sum(b);
    if constexpr (NT > kWave) {
        constexpr int NW = NT / kWave;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
            slots[wave] = a;
            slots[NW + wave] = b;
        }
        __syncthreads();
        a = slots[0];
        b = slots[NW];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            a += slots[w];
            b += slots[NW + w];
        }
    }
}

// One row of D per owner (NT = 64: wave w of workgroup blockIdx.x owns row 4 blockIdx.x + w; NT = 1024: the workgroup owns row
// blockIdx.x), chunk subspace blockIdx.y.  The row's n - 1 entries j != i are read from global memory once, into LDS, and thread t
// of the owner alone reads and writes the positions t + NT k: nothing orders the row's LDS traffic but the thread itself.
template <int NT>
__global__ __launch_bounds__(NT == kWave ? kBlock : NT) void sos_fit_kernel(const float* __restrict__ D, int n, double perplexity,
                                                                            double log_perplexity, double tol, int max_iter,
                                                                            double* __restrict__ beta, double* __restrict__ dmin,
                                                                            double* __restrict__ Z, int32_t* __restrict__ n_iter,
                                                                            int32_t* __restrict__ flags) {
    constexpr int NW = NT / kWave;
    constexpr int kCap = NT == kWave ? VGAN_SOS_WAVE_ROWS : VGAN_SOS_MAX_ROWS;  // 4 x 8 KiB or 128 KiB of the CU's 160
    __shared__ float held[(NT == kWave ? kBlock / kWave : 1) * kCap];
    __shared__ double slots[NT > kWave ? 2 * 2 * NW : 1];
    const int z = blockIdx.y;
    const int t = NT == kWave ? (threadIdx.x & 63) : threadIdx.x;
    const int i = NT == kWave ? blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6) : blockIdx.x;
    if (i >= n) return;  // a whole wave of the NT = 64 form, which has no barrier
    const float* row = D + ((long)z * n + i) * n;
    float* d = held + (NT == kWave ? (threadIdx.x >> 6) * kCap : 0);
    const int m = n - 1;  // position j holds column j + (j >= i)

    float lowest = INFINITY;
    for (int j = t; j < m; j += NT) {
        const float v = row[j + (j >= i ? 1 : 0)];
        d[j] = v;
        lowest = fminf(lowest, v);
    }
    // dmin and the number of entries equal to it: a minimum and a count, both exact
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lowest = fminf(lowest, __shfl_xor(lowest, o, 64));
    if constexpr (NT > kWave) {
        __shared__ float mins[NW];
        if ((t & 63) == 0) mins[t >> 6] = lowest;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; ++w) lowest = fminf(lowest, mins[w]);
    }
    int ties = 0;
    for (int j = t; j < m; j += NT) ties += d[j] == lowest ? 1 : 0;
    ties = wave_sum(ties);
    if constexpr (NT > kWave) {
        __shared__ int counts[NW];
        if ((t & 63) == 0) counts[t >> 6] = ties;
        __syncthreads();
        ties = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) ties += counts[w];
    }
    const double dm = (double)lowest;
    const long out = (long)z * n + i;
    if ((double)ties >= perplexity) {  // the entropy never falls to log(perplexity): uniform over the tied nearest rows
        if (t == 0) {
            beta[out] = INFINITY;
            dmin[out] = dm;
            Z[out] = (double)ties;
            n_iter[out] = 0;
            flags[out] = VGAN_SOS_FLAG_DEGENERATE;
        }
        return;
    }

    double b = 1.0, lo = 0.0, hi = INFINITY, Zs;
    int it = 0, flag = 0;
    for (;;) {
        double zs = 0.0, es = 0.0;
        // two entries a turn, unrolled by hand (the empty asm of mul_rounded keeps the compiler from doing it), added in
        // ascending j all the same
        for (int j = t; j < m; j += 2 * NT) {
            const double e0 = (double)d[j] - dm;
            if (j + NT < m) {
                const double e1 = (double)d[j + NT] - dm;
                const double a0 = exp(-mul_rounded(b, e0)), a1 = exp(-mul_rounded(b, e1));
                zs += a0;
                es += mul_rounded(e0, a0);
                zs += a1;
                es += mul_rounded(e1, a1);
            } else {
                const double a0 = exp(-mul_rounded(b, e0));
                zs += a0;
                es += mul_rounded(e0, a0);
            }
        }
        sos_sum2<NT>(zs, es, slots + (it & 1) * 2 * NW);
        Zs = zs;
        const double diff = (log(zs) + mul_rounded(b, es / zs)) - log_perplexity;
        if (fabs(diff) <= tol) break;
        if (it >= max_iter) {
            flag = VGAN_SOS_FLAG_UNCONVERGED;
            break;
        }
        if (diff > 0.0) {
            lo = b;
            b = hi == INFINITY ? 2.0 * b : (b + hi) / 2.0;
        } else {
            hi = b;
            b = (b + lo) / 2.0;
        }
        ++it;
    }
    if (t == 0) {
        beta[out] = b;
        dmin[out] = dm;
        Z[out] = Zs;
        n_iter[out] = it;
        flags[out] = flag;
    }
}

// rint(min(term, 128) 2^40) of the fitted row (beta, dmin, Z) for a row at dissimilarity d to it.  FIT: the binding probability
// b = min(a / Z, 1) and the term -log1p(-b); else the row is a new one appended to the set, b = a / (Z + a), the term log1p(a / Z).
template <bool FIT>
__device__ __forceinline__ unsigned long long sos_term(double d, double beta, double dmin, double Z) {
    double a;
    if (beta == INFINITY)
        a = d <= dmin ? 1.0 : 0.0;
    else
        a = exp(-mul_rounded(beta, d - dmin));
    const double r = a / Z;
    const double t = FIT ? -log1p(-fmin(r, 1.0)) : log1p(r);
    return (unsigned long long)(long long)rint(fmin(t, 128.0) * 0x1p40);
}

__device__ __forceinline__ float sos_score(unsigned long long sum) { return (float)exp(-((double)sum * 0x1p-40)); }

// The scores of the fitted rows from the stored matrix: wave w of workgroup blockIdx.x sums the terms of row j = 4 blockIdx.x + w
// of chunk subspace blockIdx.y over the fitted rows i != j, d_i = D[j, i].  Integer sums: any order.
__global__ __launch_bounds__(kBlock) void sos_fit_scores_kernel(const float* __restrict__ D, int n, const double* __restrict__ beta,
                                                                const double* __restrict__ dmin, const double* __restrict__ Z,
                                                                float* __restrict__ score, const int32_t* __restrict__ score_row,
                                                                long ld_score) {
    const int z = blockIdx.y, lane = threadIdx.x & 63;
    const int j = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (j >= n) return;
    const float* row = D + ((long)z * n + j) * n;
    const double* bz = beta + (long)z * n;
    const double* mz = dmin + (long)z * n;
    const double* zz = Z + (long)z * n;
    unsigned long long a = 0;
    for (int i = lane; i < n; i += kWave)
        if (i != j) a += sos_term<true>((double)row[i], bz[i], mz[i], zz[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) score[(long)(score_row ? score_row[z] : z) * ld_score + j] = sos_score(a);
}

// acc[z nq + q] += the terms of new row q over the reference rows of this slice.  Every term is at most 2^47 and nr <= 2^15, so
// the integer sum stays below 2^63.
template <bool GRAM>
__global__ __launch_bounds__(kBlock, 2) void sos_sum_kernel(const float* __restrict__ Pq, const float* __restrict__ sqq, int nq,
                                                            const float* __restrict__ Pr, const float* __restrict__ sqr, int nr,
                                                            const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                            int first, int splits, int metric, const double* __restrict__ beta,
                                                            const double* __restrict__ dmin, const double* __restrict__ Z,
                                                            unsigned long long* __restrict__ acc) {
    __shared__ __attribute__((aligned(16))) float lds[DistLds<GRAM>::kFloats];
    const int q = blockIdx.x * kOTile + (threadIdx.x & 63);
    const double* bz = beta + (long)(first + blockIdx.z) * nr;
    const double* mz = dmin + (long)(first + blockIdx.z) * nr;
    const double* zz = Z + (long)(first + blockIdx.z) * nr;
    fixed_point_row_sums<GRAM>(Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, lds, acc, [&](const float (&d2)[16], int c0) {
        unsigned long long t = 0;
        if (q >= nq) return t;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j;
            if (c < nr) t += sos_term<false>((double)sos_entry(metric, d2[j]), bz[c], mz[c], zz[c]);
        }
        return t;
    });
}

// score[score_row[z], q] = float32(exp(-(acc 2^-40))); one thread per row
__global__ void sos_score_kernel(const unsigned long long* __restrict__ acc, int nq, int count, float* __restrict__ score,
                                 const int32_t* __restrict__ score_row, long ld_score) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (long)count * nq) return;
    const int z = (int)(row / nq), q = (int)(row % nq);
    score[(long)(score_row ? score_row[z] : z) * ld_score + q] = sos_score(acc[row]);
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_sos_distance_matrix(const float* P, const float* sq, int n, const int32_t* feat_off, const int64_t* col_off,
                                        int first, int count, int metric, int engine, int splits, float* D, vgan_stream_t stream) {
    VGAN_CHECK_ARG(P && feat_off && col_off && D && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(n >= VGAN_SOS_MIN_ROWS && n <= VGAN_SOS_MAX_ROWS);
    VGAN_CHECK_ARG(metric == VGAN_SOS_METRIC_EUCLIDEAN || metric == VGAN_SOS_METRIC_SQEUCLIDEAN);
    VGAN_CHECK_ARG(dist_args_ok(engine, sq != nullptr, splits, P, P));
    launch_pair_matrix<false>(engine, P, sq, n, P, sq, n, feat_off, col_off, first, count, splits, SosEntry{metric}, D, (hipStream_t)stream);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_sos_fit(const float* D, int n, int count, double perplexity, double tol, int max_iter, int storage, double* beta,
                            double* dmin, double* Z, int32_t* n_iter, int32_t* flags, vgan_stream_t stream) {
    VGAN_CHECK_ARG(D && beta && dmin && Z && n_iter && flags && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(n >= VGAN_SOS_MIN_ROWS && n <= VGAN_SOS_MAX_ROWS);
    VGAN_CHECK_ARG(perplexity > 1.0 && perplexity < (double)(n - 1));  // false for nan
    VGAN_CHECK_ARG(tol > 0.0 && tol < INFINITY && max_iter >= 1);
    VGAN_CHECK_ARG(storage >= VGAN_SOS_STORAGE_AUTO && storage <= VGAN_SOS_STORAGE_BLOCK);
    VGAN_CHECK_ARG(storage != VGAN_SOS_STORAGE_WAVE || n <= VGAN_SOS_WAVE_ROWS);
    const hipStream_t st = (hipStream_t)stream;
    const double log_perplexity = log(perplexity);
    if (storage == VGAN_SOS_STORAGE_AUTO) storage = n <= VGAN_SOS_WAVE_ROWS ? VGAN_SOS_STORAGE_WAVE : VGAN_SOS_STORAGE_BLOCK;
    if (storage == VGAN_SOS_STORAGE_WAVE)
        hipLaunchKernelGGL(sos_fit_kernel<kWave>, dim3((n + 3) / 4, count), dim3(kBlock), 0, st, D, n, perplexity, log_perplexity, tol,
                           max_iter, beta, dmin, Z, n_iter, flags);
    else
        hipLaunchKernelGGL(sos_fit_kernel<kSosWide>, dim3(n, count), dim3(kSosWide), 0, st, D, n, perplexity, log_perplexity, tol,
                           max_iter, beta, dmin, Z, n_iter, flags);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_sos_fit_scores(const float* D, int n, int count, const double* beta, const double* dmin, const double* Z,
                                   float* score, const int32_t* score_row, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(D && beta && dmin && Z && score && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(n >= VGAN_SOS_MIN_ROWS && n <= VGAN_SOS_MAX_ROWS && ld_score >= n);
    hipLaunchKernelGGL(sos_fit_scores_kernel, dim3((n + 3) / 4, count), dim3(kBlock), 0, (hipStream_t)stream, D, n, beta, dmin, Z, score,
                       score_row, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_sos_scores(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                               const int32_t* feat_off, const int64_t* col_off, int first, int count, int metric, const double* beta,
                               const double* dmin, const double* Z, int engine, int splits, uint64_t* acc, float* score,
                               const int32_t* score_row, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Pq && Pr && feat_off && col_off && beta && dmin && Z && acc && score && nq > 0 && first >= 0);
    VGAN_CHECK_ARG(count > 0 && count <= 65535 && ld_score >= nq && nr >= VGAN_SOS_MIN_ROWS && nr <= VGAN_SOS_MAX_ROWS);
    VGAN_CHECK_ARG(metric == VGAN_SOS_METRIC_EUCLIDEAN || metric == VGAN_SOS_METRIC_SQEUCLIDEAN);
    VGAN_CHECK_ARG(dist_args_ok(engine, sq_q && sq_r, splits, Pq, Pr));
    const hipStream_t st = (hipStream_t)stream;
    const long rows = (long)count * nq;
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(acc);
    if (hipMemsetAsync(sum, 0, rows * sizeof(unsigned long long), st) != hipSuccess) {
        set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        return VGAN_ERR_HIP;
    }
    dispatch_engine(engine, [&](auto gram) {
        hipLaunchKernelGGL(sos_sum_kernel<decltype(gram)::value>, dist_grid(nq, splits, count), dim3(kBlock), 0, st, Pq, sq_q, nq, Pr, sq_r,
                           nr, feat_off, col_off, first, splits, metric, beta, dmin, Z, sum);
    });
    VGAN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sos_score_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, sum, nq, count, score, score_row,
                       (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

// One-class SVM outlier scores over the subspaces (Schoelkopf et al. 2001; sklearn's OneClassSVM with the RBF kernel, pyod's
// OCSVM; v-gan_amd/outlier.py: SubspaceOCSVM, whose docstring is the contract).
//
// Per subspace s with K_s(x, y) = exp(-gamma_s d_s(x, y)^2):
//   1. kernel matrix  outlier_dist.hpp's pair_matrix_kernel (both engines) over the packed block against itself, stored by
//                     reference row: every d2 becomes float32 exp(-gamma_s d2), the diagonal exactly 1 (RbfEntry<true>).
//   2. init           libsvm's start of the dual and G = K a, row after row.
//   3. smo            one workgroup per subspace runs WSS2 steps (Fan, Chen, Lin 2005), all float64, every operation
//                     rounded on its own; at most `iterations` steps per launch, the host polls the done flags.
//   4. rho            the mean of G over the free rows, or the midpoint / one bound where there is none.
//   5. scores         outlier_dist.hpp's fixed_point_row_sums of the query rows against the fitted rows; the terms a_r
//                     K_s(x_r, q) are summed in 64-bit fixed point (2^-44), so the sum has no order: score = rho - sum.
#include <float.h>
#include <limits.h>

#include "outlier_dist.hpp"

namespace vgan {

constexpr int kSmoLdsRows = VGAN_OCSVM_LDS_ROWS;  // up to here a and G of a subspace live in LDS during a launch (32 KiB)
constexpr int kSmoWide = 1024;  // threads of the solver's workgroup beyond that: four times fewer rows per thread and pass

// libsvm's start: a_t = 1 for t < m, a_m (when m < n), 0 beyond; G_t = sum over the nonzero rows r ascending of K[r, t] a_r.
// One thread per (subspace, t).
__global__ void ocsvm_init_kernel(const float* __restrict__ K, int n, int m, double a_m, double* __restrict__ alpha,
                                  double* __restrict__ G, int32_t* __restrict__ done, int32_t* __restrict__ n_iter) {
    const int z = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        done[z] = 0;
        n_iter[z] = 0;
    }
    if (t >= n) return;
    const float* Kz = K + (long)z * n * n;
    double g = 0.0;
    for (int r = 0; r < m; ++r) g += (double)Kz[(long)r * n + t];  // a_r = 1: the product is exact
    if (m < n && a_m != 0.0) g += mul_rounded((double)Kz[(long)m * n + t], a_m);
    alpha[(long)z * n + t] = t < m ? 1.0 : (t == m ? a_m : 0.0);
    G[(long)z * n + t] = g;
}

// (value, index) order of the two selections: the larger value, then the lower index
__device__ __forceinline__ bool smo_better(double v, int i, double w, int j) { return v > w || (v == w && i < j); }

// the best (value, index) of the NW slots a selection left in LDS, and the slot that holds it: lane l < NW takes slot l, a
// butterfly over the NW lanes, lane 0's result to every lane (NW a power of two, at most 16)
template <int NW>
__device__ __forceinline__ void smo_slots(const double* v, const int* idx, int lane, double& bv, int& bi, int& bw) {
    bv = lane < NW ? v[lane] : -INFINITY;
    bi = lane < NW ? idx[lane] : INT_MAX;
    bw = lane;
#pragma unroll
    for (int o = NW / 2; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64), ow = __shfl_xor(bw, o, 64);
        if (smo_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
            bw = ow;
        }
    }
    bv = __shfl(bv, 0, 64);
    bi = __shfl(bi, 0, 64);
    bw = __shfl(bw, 0, 64);
}

// At most `iterations` SMO steps of chunk subspace blockIdx.x by a workgroup of NT threads.  Thread tid owns the rows t =
// tid (mod NT): it alone reads and writes a_t and G_t, in LDS (LDS: n <= kSmoLdsRows) or in place, so a step needs the
// workgroup only for its two selections.  A selection is a strided pass, a wave butterfly on (value, index) and one LDS
// slot per wave, written by the lane that owns the wave's winner together with what the update needs of that row (a_i; a_j,
// G_j, K[i, j]): two barriers per step, and no thread reads a row that another one is about to write.  The strided passes
// load unconditionally and are unrolled, so that several loads of a thread are in flight.
template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void ocsvm_smo_kernel(const float* __restrict__ K, int n, double tol, int max_iter, int iterations,
                                                       double* alpha, double* G, int32_t* done, int32_t* n_iter) {
    constexpr int NW = NT / kWave;
    __shared__ double sa[LDS ? kSmoLdsRows : 1], sg[LDS ? kSmoLdsRows : 1];
    __shared__ double r1v[NW], r1a[NW], r1m[NW], r2v[NW], r2a[NW], r2g[NW];
    __shared__ float r2k[NW];
    __shared__ int r1i[NW], r2i[NW];
    const int z = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool stopped = done[z] != 0;
    __syncthreads();  // every wave has read the flag before thread 0 may set it
    if (stopped) return;
    const float* Kz = K + (long)z * n * n;
    double* ga = alpha + (long)z * n;
    double* gg = G + (long)z * n;
    double* a = LDS ? sa : ga;
    double* g = LDS ? sg : gg;
    if constexpr (LDS)
        for (int t = tid; t < n; t += NT) {
            sa[t] = ga[t];
            sg[t] = gg[t];
        }
    int it = n_iter[z], state = 0;
    for (int step = 0; step < iterations; ++step) {
        if (it >= max_iter) break;
        // 1. i: the lowest index with the largest -G_t among a_t < 1; Gmax2: the largest G_t among a_t > 0
        double bv = -INFINITY, m2 = -INFINITY;
        int bi = INT_MAX;
#pragma unroll 4
        for (int t = tid; t < n; t += NT) {
            const double at = a[t], gt = g[t];
            if (at < 1.0 && -gt > bv) {
                bv = -gt;
                bi = t;
            }
            if (at > 0.0 && gt > m2) m2 = gt;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64), om = __shfl_xor(m2, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (smo_better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
            m2 = om > m2 ? om : m2;
        }
        if (bi == INT_MAX ? lane == 0 : (bi & (NT - 1)) == tid) {
            r1v[wave] = bv;
            r1i[wave] = bi;
            r1a[wave] = bi == INT_MAX ? 0.0 : a[bi];
            r1m[wave] = m2;
        }
        __syncthreads();
        double Gmax, Gmax2 = lane < NW ? r1m[lane] : -INFINITY;
        int i, iw;
        smo_slots<NW>(r1v, r1i, lane, Gmax, i, iw);
#pragma unroll
        for (int o = NW / 2; o > 0; o >>= 1) {
            const double om = __shfl_xor(Gmax2, o, 64);
            Gmax2 = om > Gmax2 ? om : Gmax2;
        }
        Gmax2 = __shfl(Gmax2, 0, 64);
        // 2. the stop rule
        if (i == INT_MAX || Gmax + Gmax2 < tol) {
            state = 1;
            break;
        }
        const double a_i = r1a[iw];
        // 3. j: the lowest index with the smallest -(b_t^2) / q_t among a_t > 0, b_t = Gmax + G_t > 0
        const float* Ki = Kz + (long)i * n;
        double cv = -INFINITY;  // the largest b^2 / q, that is the smallest -(b^2) / q: negation is exact
        int cj = INT_MAX;
#pragma unroll 4
        for (int t = tid; t < n; t += NT) {
            const double at = a[t], gt = g[t], kt = (double)Ki[t];
            const double b = Gmax + gt;
            double q = 2.0 - 2.0 * kt;
            if (q <= 0.0) q = 1e-12;
            const double obj = (b * b) / q;
            if (at > 0.0 && b > 0.0 && obj > cv) {
                cv = obj;
                cj = t;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(cv, o, 64);
            const int oj = __shfl_xor(cj, o, 64);
            if (smo_better(ov, oj, cv, cj)) {
                cv = ov;
                cj = oj;
            }
        }
        if (cj == INT_MAX ? lane == 0 : (cj & (NT - 1)) == tid) {
            r2v[wave] = cv;
            r2i[wave] = cj;
            if (cj != INT_MAX) {
                r2a[wave] = a[cj];
                r2g[wave] = g[cj];
                r2k[wave] = Ki[cj];
            }
        }
        __syncthreads();
        double jv;
        int j, jw;
        smo_slots<NW>(r2v, r2i, lane, jv, j, jw);
        if (j == INT_MAX) {
            state = 1;
            break;
        }
        // 4. the update of the pair, libsvm's clips for equal labels with C = 1
        const double a_j = r2a[jw], G_j = r2g[jw], G_i = -Gmax;
        double q = 2.0 - 2.0 * (double)r2k[jw];
        if (q <= 0.0) q = 1e-12;
        const double delta = (G_i - G_j) / q, sum = a_i + a_j;
        double ai = a_i - delta, aj = a_j + delta;
        if (sum > 1.0) {
            if (ai > 1.0) {
                ai = 1.0;
                aj = sum - 1.0;
            }
        } else if (aj < 0.0) {
            aj = 0.0;
            ai = sum;
        }
        if (sum > 1.0) {
            if (aj > 1.0) {
                aj = 1.0;
                ai = sum - 1.0;
            }
        } else if (ai < 0.0) {
            ai = 0.0;
            aj = sum;
        }
        const double dai = ai - a_i, daj = aj - a_j;
        if ((i & (NT - 1)) == tid) a[i] = ai;
        if ((j & (NT - 1)) == tid) a[j] = aj;
        // 5. G_t += K[i, t] da_i + K[j, t] da_j: two rounded products, their rounded sum, then the sum with G_t
        const float* Kj = Kz + (long)j * n;
        // (four rows a turn, unrolled by hand: the empty asm of mul_rounded keeps the compiler from doing it)
        for (int t0 = tid; t0 < n; t0 += 4 * NT) {
            float ki[4], kj[4];
            double gv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + u * NT;
                if (t < n) {
                    ki[u] = Ki[t];
                    kj[u] = Kj[t];
                    gv[u] = g[t];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + u * NT;
                if (t < n) g[t] = gv[u] + (mul_rounded((double)ki[u], dai) + mul_rounded((double)kj[u], daj));
            }
        }
        ++it;
    }
    if (state == 0 && it >= max_iter) state = 2;
    if constexpr (LDS)
        for (int t = tid; t < n; t += NT) {
            ga[t] = sa[t];
            gg[t] = sg[t];
        }
    if (tid == 0) {
        n_iter[z] = it;
        if (state != 0) done[z] = state;
    }
}

// rho of chunk subspace blockIdx.x: a fixed order (strided per thread, the wave butterfly, the four waves in order)
__global__ __launch_bounds__(kBlock) void ocsvm_rho_kernel(const double* __restrict__ alpha, const double* __restrict__ G, int n,
                                                           double* __restrict__ rho) {
    __shared__ double red[4], rlb[4], rub[4];
    __shared__ int rcount[4];
    const int z = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* a = alpha + (long)z * n;
    const double* g = G + (long)z * n;
    double sum = 0.0, lb = -INFINITY, ub = INFINITY;
    int count = 0;
    for (int t = tid; t < n; t += kBlock) {
        const double at = a[t], gt = g[t];
        if (at >= 1.0) {
            lb = gt > lb ? gt : lb;
        } else if (at <= 0.0) {
            ub = gt < ub ? gt : ub;
        } else {
            sum += gt;
            ++count;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ol = __shfl_xor(lb, o, 64), ou = __shfl_xor(ub, o, 64);
        lb = ol > lb ? ol : lb;
        ub = ou < ub ? ou : ub;
    }
    count = wave_sum(count);
    if (lane == 0) {
        rlb[wave] = lb;
        rub[wave] = ub;
        rcount[wave] = count;
    }
    sum = block_sum(sum, red);  // its barrier covers the three arrays above too
    if (tid != 0) return;
    for (int w = 1; w < 4; ++w) {  // lb, ub: wave 0's
        lb = rlb[w] > lb ? rlb[w] : lb;
        ub = rub[w] < ub ? rub[w] : ub;
    }
    count = rcount[0] + rcount[1] + rcount[2] + rcount[3];
    double r;
    if (count > 0)
        r = sum / (double)count;
    else if (lb > -INFINITY && ub < INFINITY)
        r = (ub + lb) / 2.0;
    else
        r = lb > -INFINITY ? lb : ub;
    rho[z] = r;
}

// acc[z nq + q] += sum over the reference rows r of this slice with a_r != 0 of rint(a_r K_s(x_r, q) 2^44): every term lies
// in [0, 2^44] and nr <= 2^15, so the integer sum stays below 2^63 and has no order
template <bool GRAM>
__global__ __launch_bounds__(kBlock, 2) void ocsvm_sum_kernel(const float* __restrict__ Pq, const float* __restrict__ sqq, int nq,
                                                              const float* __restrict__ Pr, const float* __restrict__ sqr, int nr,
                                                              const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                              int first, int splits, const double* __restrict__ gamma,
                                                              const double* __restrict__ alpha, unsigned long long* __restrict__ acc) {
    __shared__ __attribute__((aligned(16))) float lds[DistLds<GRAM>::kFloats];
    const int q = blockIdx.x * kOTile + (threadIdx.x & 63);
    const double g = gamma[first + blockIdx.z];
    const double* az = alpha + (long)(first + blockIdx.z) * nr;
    fixed_point_row_sums<GRAM>(Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, lds, acc, [&](const float (&d2)[16], int c0) {
        unsigned long long t = 0;
        if (q >= nq) return t;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j;
            if (c >= nr) continue;
            const double w = az[c];
            if (w != 0.0) t += (unsigned long long)(long long)rint(mul_rounded(w, (double)rbf_entry(g, d2[j])) * 0x1p44);
        }
        return t;
    });
}

// score[score_row[z], q] = float32((rint(rho 2^44) - acc) 2^-44): rho enters on the grid of the sum, so that equal terms cancel
// exactly; one thread per row
__global__ void ocsvm_score_kernel(const unsigned long long* __restrict__ acc, int nq, int count, int first,
                                   const double* __restrict__ rho, float* __restrict__ score, const int32_t* __restrict__ score_row,
                                   long ld_score) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (long)count * nq) return;
    const int z = (int)(row / nq), q = (int)(row % nq);
    const long long r = (long long)rint(rho[first + z] * 0x1p44);
    score[(long)(score_row ? score_row[z] : z) * ld_score + q] = (float)((double)(r - (long long)acc[row]) * 0x1p-44);
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_ocsvm_kernel_matrix(const float* P, const float* sq, int n, const int32_t* feat_off, const int64_t* col_off,
                                        int first, int count, const double* gamma, int engine, int splits, float* K,
                                        vgan_stream_t stream) {
    VGAN_CHECK_ARG(P && feat_off && col_off && gamma && K && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(n >= 2 && n <= VGAN_OCSVM_MAX_ROWS);
    VGAN_CHECK_ARG(dist_args_ok(engine, sq != nullptr, splits, P, P));
    launch_pair_matrix<false>(engine, P, sq, n, P, sq, n, feat_off, col_off, first, count, splits, RbfEntry<true>{gamma}, K,
                              (hipStream_t)stream);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ocsvm_init(const float* K, int n, int count, int m, double a_m, double* alpha, double* G, int32_t* done,
                               int32_t* n_iter, vgan_stream_t stream) {
    VGAN_CHECK_ARG(K && alpha && G && done && n_iter && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(n >= 2 && n <= VGAN_OCSVM_MAX_ROWS && m >= 0 && m <= n);
    VGAN_CHECK_ARG(m < n ? (a_m >= 0.0 && a_m < 1.0) : a_m == 0.0);  // false for nan
    VGAN_CHECK_ARG(m > 0 || a_m > 0.0);
    hipLaunchKernelGGL(ocsvm_init_kernel, dim3((n + 255) / 256, count), dim3(256), 0, (hipStream_t)stream, K, n, m, a_m, alpha, G, done,
                       n_iter);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ocsvm_smo(const float* K, int n, int count, double tol, int max_iter, int iterations, int storage, double* alpha,
                              double* G, int32_t* done, int32_t* n_iter, vgan_stream_t stream) {
    VGAN_CHECK_ARG(K && alpha && G && done && n_iter && count > 0);
    VGAN_CHECK_ARG(n >= 2 && n <= VGAN_OCSVM_MAX_ROWS && tol > 0.0 && max_iter >= 1 && iterations >= 1);
    VGAN_CHECK_ARG(storage >= VGAN_OCSVM_STORAGE_AUTO && storage <= VGAN_OCSVM_STORAGE_WIDE);
    VGAN_CHECK_ARG(storage != VGAN_OCSVM_STORAGE_LDS || n <= VGAN_OCSVM_LDS_ROWS);
    const hipStream_t st = (hipStream_t)stream;
    if (storage == VGAN_OCSVM_STORAGE_AUTO) storage = n <= VGAN_OCSVM_LDS_ROWS ? VGAN_OCSVM_STORAGE_LDS : VGAN_OCSVM_STORAGE_WIDE;
    if (storage == VGAN_OCSVM_STORAGE_LDS)
        hipLaunchKernelGGL((ocsvm_smo_kernel<kBlock, true>), dim3(count), dim3(kBlock), 0, st, K, n, tol, max_iter, iterations, alpha, G,
                           done, n_iter);
    else if (storage == VGAN_OCSVM_STORAGE_GLOBAL)
        hipLaunchKernelGGL((ocsvm_smo_kernel<kBlock, false>), dim3(count), dim3(kBlock), 0, st, K, n, tol, max_iter, iterations, alpha, G,
                           done, n_iter);
    else
        hipLaunchKernelGGL((ocsvm_smo_kernel<kSmoWide, false>), dim3(count), dim3(kSmoWide), 0, st, K, n, tol, max_iter, iterations, alpha,
                           G, done, n_iter);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ocsvm_rho(const double* alpha, const double* G, int n, int count, double* rho, vgan_stream_t stream) {
    VGAN_CHECK_ARG(alpha && G && rho && count > 0 && n >= 2 && n <= VGAN_OCSVM_MAX_ROWS);
    hipLaunchKernelGGL(ocsvm_rho_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, alpha, G, n, rho);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ocsvm_scores(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                                 const int32_t* feat_off, const int64_t* col_off, int first, int count, const double* gamma,
                                 const double* alpha, const double* rho, int engine, int splits, uint64_t* acc, float* score,
                                 const int32_t* score_row, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Pq && Pr && feat_off && col_off && gamma && alpha && rho && acc && score && nq > 0 && first >= 0);
    VGAN_CHECK_ARG(count > 0 && count <= 65535 && ld_score >= nq && nr >= 2 && nr <= VGAN_OCSVM_MAX_ROWS);
    VGAN_CHECK_ARG(dist_args_ok(engine, sq_q && sq_r, splits, Pq, Pr));
    const hipStream_t st = (hipStream_t)stream;
    const long rows = (long)count * nq;
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(acc);
    if (hipMemsetAsync(sum, 0, rows * sizeof(unsigned long long), st) != hipSuccess) {
        set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        return VGAN_ERR_HIP;
    }
    dispatch_engine(engine, [&](auto gram) {
        hipLaunchKernelGGL(ocsvm_sum_kernel<decltype(gram)::value>, dist_grid(nq, splits, count), dim3(kBlock), 0, st, Pq, sq_q, nq, Pr, sq_r,
                           nr, feat_off, col_off, first, splits, gamma, alpha, sum);
    });
    VGAN_CHECK_LAUNCH();
    hipLaunchKernelGGL(ocsvm_score_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, sum, nq, count, first, rho, score,
                       score_row, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

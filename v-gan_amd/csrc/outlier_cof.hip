// Connectivity-based outlier scores (COF: Tang, Chen, Fu, Cheung 2002; pyod's COF) over the refined neighbour lists of
// outlier.hip.  Per (subspace s, query row q) with the listed reference rows o_1 .. o_k (k <= 32, list order) and o_0 = q:
//   d2(a, b) = sum_{f in F_s} (x_a[f] - x_b[f])^2 in float64 from the raw float32 values, features ascending, for all pairs
//              of the k + 1 points.  The difference is taken per feature; the Gram form n_a + n_b - 2 G_ab is not used, its
//              cancellation costs exactly the small distances that decide the chain
//   chain sbn  the set starts as {o_0}; step i = 1 .. k adds the remaining point with the smallest (d2 to the set, list
//              position), d2 to the set being the minimum over the set's members; e_i = sqrt of that d2
//   chain rank e_i = sqrt(min_{j < i} d2(o_i, o_j)): the points in list order, nothing is selected
//   ac(q) = sum_{i = 1 .. k} w_i e_i, w_i = 2 (k + 1 - i) / (k (k + 1)), float64, i ascending
// The score kernel forms ac(q) k / sum_i ac_ref(o_i), the fill kernel of outlier_nbr.hpp puts the ceiling into the degenerate rows.
//
// The chain kernel is the layout of outlier_nbr.hpp (one wave per item, lane (I, J) owns a T x T block of pairs) with a
// selection behind it.
//   stage    the raw values (exact in float64), the query's in the pad slot.  The slot of a missing neighbour holds 0 and is
//            never selected
//   pairs    per feature 2 T + 2 doubles from LDS, T^2 subtractions and multiply-adds for the block and one for the
//            query-to-neighbour vector: the lane forms the entry of row T I + J % T, the lanes J < T publish theirs.
//            (a - b)^2 and (b - a)^2 are the same float64, so the matrix is symmetric to the bit
//   matrix   after the feature loop the k x k d2 matrix goes to LDS over the staging buffer ([KP][KP] doubles, 8 KB per
//            wave at KP = 32 against the buffer's 8.5 KB), the query vector next to it
//   chain    lane l < k holds the d2 of point l + 1 to the set.  A step is a wave minimum on the bit pattern (d2 >= 0, so
//            the IEEE bits order like the values), a ballot for the lowest lane that holds it, and one LDS row read that
//            updates every remaining lane; the weighted sum runs wave-uniform in step order.  No atomics anywhere.
#include <float.h>

#include "outlier_nbr.hpp"

namespace vgan {

template <int T>
struct CofPairs {
    static constexpr bool kQueryInPad = true, kListInLds = true;
    static constexpr int KP = NbrItem<T>::KP;
    const int aq;  // the neighbour whose distance to the query this lane forms: row T I + J % T (lanes J < T publish it)
    double acc[T][T] = {}, accq = 0.0;
    __device__ explicit CofPairs(int lane) : aq(T * (lane >> 3) + (lane & (T - 1))) {}
    static __device__ __forceinline__ double stage(float r, float) { return (double)r; }
    __device__ __forceinline__ void update(const double* row, const double (&av)[T], const double (&bv)[T]) {
        const double dq = row[aq] - row[KP];
        accq = fma(dq, dq, accq);
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const double df = av[i] - bv[j];
                acc[i][j] = fma(df, df, acc[i][j]);
            }
    }
};

template <int T, bool SBN>
__global__ __launch_bounds__(kBlock, 4) void outlier_cof_chain_kernel(NbrArgs g, double* __restrict__ ac_out) {
    constexpr int KP = NbrItem<T>::KP;
    static_assert(KP * KP <= kNbrFB * NbrItem<T>::LD, "the d2 matrix reuses the staging buffer");
    __shared__ double lds_q[kNbrWaves][KP];
    CofPairs<T> d2(threadIdx.x & 63);
    const NbrItem<T> it = nbr_pair_blocks<T>(g, d2);
    const int k = g.k, lane = it.lane, wave = it.wave, I = it.I, J = it.J;
    double* V = it.V;

    // the d2 matrix over the staging buffer, the query-to-neighbour vector next to it
    __syncthreads();
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) V[(T * I + i) * KP + T * J + j] = d2.acc[i][j];
    if (J < T) lds_q[wave][d2.aq] = d2.accq;
    __syncthreads();

    // lane l < k: the d2 of point l + 1 to the set, as its bit pattern; a point in the set is no longer `rem`
    bool rem = lane < k;
    double dist = rem ? lds_q[wave][lane] : 0.0;
    const double wden = (double)(k * (k + 1));
    double ac = 0.0;
    for (int i = 1; i <= k; ++i) {
        int j;
        unsigned long long mbits;
        if (SBN) {
            const unsigned long long bits = rem ? (unsigned long long)__double_as_longlong(dist) : ~0ull;
            mbits = ~wave_max(~bits);
            const unsigned long long holders = __ballot(rem && bits == mbits);
            j = holders ? __ffsll((long long)holders) - 1 : 0;
        } else {
            j = i - 1;
            mbits = (unsigned long long)__shfl(__double_as_longlong(dist), j, 64);
        }
        const double e = sqrt(__longlong_as_double((long long)mbits));
        ac += (double)(2 * (k + 1 - i)) / wden * e;
        if (lane == j) rem = false;
        const double dj = V[j * KP + (lane < KP ? lane : 0)];
        if (rem && dj < dist) dist = dj;
    }
    if (lane == 0 && it.q_raw < g.nq) ac_out[(long)it.z * g.nq + it.q] = ac;
}

// score[row, q] = ac_q[z, q] k / sum_{i = 1 .. k} ac_ref[z, idx[z, q, i]], float64, i ascending, one thread per (z, q).
// A zero denominator: 1 where ac_q is 0 too (a point mass among point masses), NaN otherwise (DEGENERATE: the ceiling kernel
// fills it in).  A value beyond the float32 range is stored as FLT_MAX.
__global__ __launch_bounds__(kBlock) void outlier_cof_score_kernel(const double* __restrict__ ac_q, int nq,
                                                                   const double* __restrict__ ac_ref, int nr,
                                                                   const int32_t* __restrict__ idx, int k,
                                                                   float* __restrict__ score, const int32_t* __restrict__ score_row,
                                                                   int ld_score) {
    const int z = blockIdx.y, q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= nq) return;
    const int32_t* list = idx + ((long)z * nq + q) * k;
    const double* ref = ac_ref + (long)z * nr;
    double den = 0.0;
    for (int i = 0; i < k; ++i) {
        const int r = list[i];
        den += (unsigned)r < (unsigned)nr ? ref[r] : 0.0;
    }
    const double ac = ac_q[(long)z * nq + q];
    float out;
    if (den == 0.0) {
        out = ac == 0.0 ? 1.f : NAN;
    } else {
        out = (float)(ac * (double)k / den);
        if (out == INFINITY) out = FLT_MAX;
    }
    score[(long)(score_row ? score_row[z] : z) * ld_score + q] = out;
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_outlier_cof_chain(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                                      const int32_t* feat_off, int first, int count, const int32_t* idx, int k, int chain,
                                      double* ac_out, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && Xr && feat && feat_off && idx && ac_out && nq > 0 && nr > 0 && d > 0);
    VGAN_CHECK_ARG(ldq >= d && ldr >= d && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(k >= 1 && k <= VGAN_OUTLIER_MAX_K && nr >= k);
    VGAN_CHECK_ARG(chain == VGAN_OUTLIER_COF_CHAIN_SBN || chain == VGAN_OUTLIER_COF_CHAIN_RANK);
    const NbrArgs g{Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k};
    dispatch_nbr_tile(k, [&](auto t) {
        constexpr int T = decltype(t)::value;
        const auto kernel = chain == VGAN_OUTLIER_COF_CHAIN_SBN ? outlier_cof_chain_kernel<T, true> : outlier_cof_chain_kernel<T, false>;
        hipLaunchKernelGGL(kernel, nbr_grid(nq, count), dim3(kBlock), 0, (hipStream_t)stream, g, ac_out);
    });
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_cof_score(const double* ac_q, int nq, const double* ac_ref, int nr, const int32_t* idx, int k, int count,
                                      float* score, const int32_t* score_row, int ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(ac_q && ac_ref && idx && score && nq > 0 && nr > 0 && count > 0 && count <= 65535 && ld_score >= nq);
    VGAN_CHECK_ARG(k >= 1 && k <= VGAN_OUTLIER_MAX_K && nr >= k);
    hipLaunchKernelGGL(outlier_cof_score_kernel, dim3((nq + kBlock - 1) / kBlock, count), dim3(kBlock), 0, (hipStream_t)stream, ac_q,
                       nq, ac_ref, nr, idx, k, score, score_row, ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_cof_ceiling(float* score, int ld, int S, int n, int fit, double* score_ceiling, int32_t* n_degenerate,
                                        vgan_stream_t stream) {
    VGAN_CHECK_ARG(score && score_ceiling && S > 0 && n > 0 && ld >= n);
    VGAN_CHECK_ARG(!fit || n_degenerate);
    launch_fill_degenerate<true>(score, ld, S, n, fit, score_ceiling, n_degenerate, stream);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

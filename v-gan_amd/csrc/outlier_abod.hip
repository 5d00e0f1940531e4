// Angle-based outlier scores (FastABOD: Kriegel, Schubert, Zimek 2008; pyod's ABOD with method="fast") over the refined
// neighbour lists of outlier.hip.  Per (subspace s, query row q) with neighbours N(q) (k <= 32 reference rows):
//   v_a = r_a[F_s] - q[F_s] in float64 from the raw float32 values (exact), n_a = |v_a|^2; a is usable if n_a > 0
//   w_ab = <v_a, v_b> / (n_a n_b) for every unordered pair of usable neighbours
//   score = -var(w), population variance, two passes (mean, then mean squared deviation), float64, fixed order
// A row with no pair (fewer than two usable neighbours) is DEGENERATE: its score is written as NaN, the marker the fill
// kernel of outlier_nbr.hpp replaces by the floor of the subspace.
//
// The work of an item is a tiny SYRK: a gathered [k, d_s] float64 operand and its k x k Gram matrix, on the layout of
// outlier_nbr.hpp (one wave per item, lane (I, J) owns a T x T block of pairs).
//   stage    the differences v_a.  The slot of a missing neighbour holds 0, which makes it unusable without a special case
//   Gram     T^2 multiply-adds per feature; T = 4 keeps 16 float64 accumulators (32 VGPRs) per lane
//   variance the diagonal lanes publish the k norms through LDS; every lane forms the w of its pairs a < b, and the two
//            sums run lane-local in fixed order and then through the wave butterfly.  No atomics anywhere.
#include <float.h>

#include "outlier_nbr.hpp"

namespace vgan {

template <int T>
struct AbodPairs {
    static constexpr bool kQueryInPad = false, kListInLds = false;
    double acc[T][T] = {};
    static __device__ __forceinline__ double stage(float r, float q) { return (double)r - (double)q; }
    __device__ __forceinline__ void update(const double*, const double (&av)[T], const double (&bv)[T]) {
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
    }
};

template <int T>
__global__ __launch_bounds__(kBlock, 4) void outlier_abod_kernel(NbrArgs g, float* __restrict__ score,
                                                              const int32_t* __restrict__ score_row, int ld_score) {
    constexpr int KP = NbrItem<T>::KP;
    __shared__ double lds_n[kNbrWaves][KP];
    AbodPairs<T> gram;
    const NbrItem<T> it = nbr_pair_blocks<T>(g, gram);
    const int wave = it.wave, I = it.I, J = it.J;
    const auto& acc = gram.acc;

    // the k squared norms are the diagonal
    if (I == J) {
#pragma unroll
        for (int i = 0; i < T; ++i) lds_n[wave][T * I + i] = acc[i][i];
    }
    __syncthreads();
    double w[T][T], sum = 0.0;
    int pairs = 0;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int a = T * I + i, b = T * J + j;
            const double na = lds_n[wave][a], nbn = lds_n[wave][b];
            const bool ok = a < b && na > 0.0 && nbn > 0.0;
            w[i][j] = ok ? acc[i][j] / (na * nbn) : 0.0;
            sum += w[i][j];
            pairs += ok ? 1 : 0;
            if (!ok) w[i][j] = NAN;  // marks the slot as unused for the second pass
        }
    pairs = wave_sum(pairs);
    const double mean = wave_sum(sum) / (double)pairs;
    double dev = 0.0;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const double e = w[i][j] - mean;
            dev += w[i][j] == w[i][j] ? e * e : 0.0;
        }
    const double var = wave_sum(dev) / (double)pairs;
    if (it.lane == 0 && it.q_raw < g.nq) {
        float out = NAN;  // no pair: degenerate, the fill kernel puts the floor in
        if (pairs > 0) {
            out = (float)(0.0 - var);
            if (out == -INFINITY) out = -FLT_MAX;
        }
        score[(long)(score_row ? score_row[it.z] : it.z) * ld_score + it.q] = out;
    }
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_outlier_abod(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                                 const int32_t* feat_off, int first, int count, const int32_t* idx, int k, float* score,
                                 const int32_t* score_row, int ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && Xr && feat && feat_off && idx && score && nq > 0 && nr > 0 && d > 0);
    VGAN_CHECK_ARG(ldq >= d && ldr >= d && first >= 0 && count > 0 && count <= 65535 && ld_score >= nq);
    VGAN_CHECK_ARG(k >= 2 && k <= VGAN_OUTLIER_MAX_K && nr >= k);
    const NbrArgs g{Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k};
    dispatch_nbr_tile(k, [&](auto t) {
        hipLaunchKernelGGL(outlier_abod_kernel<decltype(t)::value>, nbr_grid(nq, count), dim3(kBlock), 0, (hipStream_t)stream, g, score,
                           score_row, ld_score);
    });
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_abod_floor(float* score, int ld, int S, int n, int fit, double* score_floor, int32_t* n_degenerate,
                                       vgan_stream_t stream) {
    VGAN_CHECK_ARG(score && score_floor && S > 0 && n > 0 && ld >= n);
    VGAN_CHECK_ARG(!fit || n_degenerate);
    launch_fill_degenerate<false>(score, ld, S, n, fit, score_floor, n_degenerate, stream);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

// Angle-based outlier scores (FastABOD: Kriegel, Schubert, Zimek 2008; pyod's ABOD with method="fast") over the refined
// neighbour lists of outlier.hip.  Per (subspace s, query row q) with neighbours N(q) (k <= 32 reference rows):
//   v_a = r_a[F_s] - q[F_s] in float64 from the raw float32 values (exact), n_a = |v_a|^2; a is usable if n_a > 0
//   w_ab = <v_a, v_b> / (n_a n_b) for every unordered pair of usable neighbours
//   score = -var(w), population variance, two passes (mean, then mean squared deviation), float64, fixed order
// A row with no pair (fewer than two usable neighbours) is DEGENERATE: its score is written as NaN, the marker the floor
// kernel below replaces by the floor of the subspace.
//
// The work of an item is a tiny SYRK: a gathered [k, d_s] float64 operand and its k x k Gram matrix.  One wave owns one
// item, a workgroup four query rows of one subspace (all four waves walk the same d_s, so the block barriers are uniform).
//   gather   F_s is walked in blocks of kAbodFB = 32 features.  The k x 32 elements of a block are spread over the lanes
//            feature-fastest (lane -> feature lane % W, neighbour lane / W + (64 / W) t; W = 32, or the next power of two
//            >= d_s in a narrower subspace), so the lanes of a load read neighbouring features of one reference row and a
//            2-feature subspace still fills the wave with 32 neighbours.  The loads of block i + 1 are issued before the
//            Gram step of block i and land in registers.
//   stage    the differences go to LDS as float64, feature-major ([32][KP + 2] per wave, KP = 8 T the padded k; the pad
//            of one 16-byte access keeps the rows off a power-of-two stride).  Slots of missing neighbours (a >= k, or
//            an index outside the reference set) hold 0, which makes them unusable without a special case.
//   Gram     lane (I, J) = (lane / 8, lane % 8) owns the T x T block of pairs (T I + i, T J + j) (T = 1, 2, 4 for k <= 8,
//            16, 32): per feature it reads 2 T doubles from LDS (one or two 16-byte reads per operand, every address
//            shared by eight lanes) for T^2 multiply-adds, features in ascending order.  The whole matrix is formed,
//            not the upper triangle: the lanes below the diagonal would idle otherwise, their cost is the same wave
//            instruction.  T = 4 keeps 16 float64 accumulators (32 VGPRs) per lane.
//   variance the diagonal lanes publish the k norms through LDS; every lane forms the w of its pairs a < b, and the two
//            sums run lane-local in fixed order and then through the wave butterfly.  No atomics anywhere.
#include <float.h>

#include "vgan_common.hpp"

namespace vgan {

constexpr int kAbodFB = 32;                       // features per staged block
constexpr int kAbodWaves = kBlock / kWave;        // items (query rows) per workgroup

template <int T>
__global__ __launch_bounds__(kBlock, 4) void outlier_abod_kernel(const float* __restrict__ Xq, int ldq, int nq,
                                                              const float* __restrict__ Xr, int ldr, int nr,
                                                              const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                              int first, const int32_t* __restrict__ idx, int k,
                                                              float* __restrict__ score, const int32_t* __restrict__ score_row,
                                                              int ld_score) {
    constexpr int KP = 8 * T, LD = KP + 2;
    constexpr int NE = KP * kAbodFB / kWave;  // staged elements per lane and feature block
    __shared__ __attribute__((aligned(16))) double lds_v[kAbodWaves][kAbodFB * LD];
    __shared__ double lds_n[kAbodWaves][KP];

    const int z = blockIdx.y, s = first + z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q_raw = blockIdx.x * kAbodWaves + wave;
    const int q = min(q_raw, nq - 1);  // a surplus wave repeats the last row (barriers stay uniform) and stores nothing
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0;
    double* V = lds_v[wave];

    // lanes over (neighbour, feature), feature fastest: W features side by side, 64 / W neighbours per load
    int logw = 5;
    while (logw > 0 && (1 << (logw - 1)) >= ds) --logw;
    const int W = 1 << logw, c = lane & (W - 1), a0 = lane >> logw, astep = kWave >> logw;

    // the reference row of each of this lane's neighbour slots (-1: none)
    const int32_t* list = idx + ((long)z * nq + q) * k;
    int nb[NE];
#pragma unroll
    for (int t = 0; t < NE; ++t) {
        const int a = a0 + t * astep;
        int r = a < k ? list[a] : -1;
        nb[t] = (unsigned)r < (unsigned)nr ? r : -1;
    }
    const float* xq = Xq + (long)q * ldq;

    // every load is unconditional inside a wave-uniform guard (slots past k are skipped by the whole wave); a lane past
    // d_s or on a missing neighbour reads a valid address again and its value is dropped when the block is staged
    float qv = 0.f, rv[NE];
    bool live = false;
#pragma unroll
    for (int t = 0; t < NE; ++t) rv[t] = 0.f;
    auto load_block = [&](int cb) {
        live = cb + c < ds;
        const int f = feat[f0 + min(cb + c, ds - 1)];
        qv = xq[f];
#pragma unroll
        for (int t = 0; t < NE; ++t)
            if (t * astep < k) rv[t] = Xr[(long)max(nb[t], 0) * ldr + f];
    };

    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = 0.0;
    const int I = lane >> 3, J = lane & 7;

    load_block(0);
    for (int cb = 0; cb < ds; cb += kAbodFB) {
        __syncthreads();  // the Gram step of the previous block has read its LDS
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int a = a0 + t * astep;
            if (a < KP) V[c * LD + a] = (live && nb[t] >= 0) ? (double)rv[t] - (double)qv : 0.0;
        }
        __syncthreads();
        if (cb + kAbodFB < ds) load_block(cb + kAbodFB);
        const int cw = min(kAbodFB, ds - cb);
        for (int f = 0; f < cw; ++f) {
            const double* row = V + f * LD;
            double av[T], bv[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                av[i] = row[T * I + i];
                bv[i] = row[T * J + i];
            }
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
        }
    }

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
    if (lane == 0 && q_raw < nq) {
        float out = NAN;  // no pair: degenerate, the floor kernel fills it in
        if (pairs > 0) {
            out = (float)(0.0 - var);
            if (out == -INFINITY) out = -FLT_MAX;
        }
        score[(long)(score_row ? score_row[z] : z) * ld_score + q] = out;
    }
}

// One workgroup per row s of the score matrix [S, ld] (n scores a row).  A NaN score marks a degenerate row.
//   fit != 0  score_floor[s] = the smallest score that is not NaN (0 if there is none), n_degenerate[s] = the number of NaNs
//   then every NaN of the row becomes (float)score_floor[s].  A minimum and an integer count are order-free.
__global__ __launch_bounds__(kBlock) void outlier_abod_floor_kernel(float* __restrict__ score, int ld, int n, int fit,
                                                                    double* __restrict__ score_floor, int32_t* __restrict__ n_degenerate) {
    __shared__ float red_m[kBlock / kWave];
    __shared__ int red_c[kBlock / kWave];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* row = score + (long)s * ld;
    float fl;
    if (fit) {
        float m = INFINITY;
        int cnt = 0;
        for (int i = tid; i < n; i += kBlock) {
            const float v = row[i];
            if (v == v) m = fminf(m, v);
            else ++cnt;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
        cnt = wave_sum(cnt);
        if (lane == 0) {
            red_m[wave] = m;
            red_c[wave] = cnt;
        }
        __syncthreads();
        m = fminf(fminf(red_m[0], red_m[1]), fminf(red_m[2], red_m[3]));
        cnt = red_c[0] + red_c[1] + red_c[2] + red_c[3];
        fl = cnt == n ? 0.f : m;
        if (tid == 0) {
            score_floor[s] = (double)fl;
            n_degenerate[s] = cnt;
        }
    } else {
        fl = (float)score_floor[s];
    }
    for (int i = tid; i < n; i += kBlock) {
        const float v = row[i];
        if (!(v == v)) row[i] = fl;
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
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((nq + kAbodWaves - 1) / kAbodWaves, count);
    if (k <= 8)
        hipLaunchKernelGGL(outlier_abod_kernel<1>, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k,
                           score, score_row, ld_score);
    else if (k <= 16)
        hipLaunchKernelGGL(outlier_abod_kernel<2>, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k,
                           score, score_row, ld_score);
    else
        hipLaunchKernelGGL(outlier_abod_kernel<4>, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k,
                           score, score_row, ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_abod_floor(float* score, int ld, int S, int n, int fit, double* score_floor, int32_t* n_degenerate,
                                       vgan_stream_t stream) {
    VGAN_CHECK_ARG(score && score_floor && S > 0 && n > 0 && ld >= n);
    VGAN_CHECK_ARG(!fit || n_degenerate);
    hipLaunchKernelGGL(outlier_abod_floor_kernel, dim3(S), dim3(kBlock), 0, (hipStream_t)stream, score, ld, n, fit ? 1 : 0, score_floor,
                       n_degenerate);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

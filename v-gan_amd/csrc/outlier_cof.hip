// Connectivity-based outlier scores (COF: Tang, Chen, Fu, Cheung 2002; pyod's COF) over the refined neighbour lists of
// outlier.hip.  Per (subspace s, query row q) with the listed reference rows o_1 .. o_k (k <= 32, list order) and o_0 = q:
//   d2(a, b) = sum_{f in F_s} (x_a[f] - x_b[f])^2 in float64 from the raw float32 values, features ascending, for all pairs
//              of the k + 1 points.  The difference is taken per feature; the Gram form n_a + n_b - 2 G_ab is not used, its
//              cancellation costs exactly the small distances that decide the chain
//   chain sbn  the set starts as {o_0}; step i = 1 .. k adds the remaining point with the smallest (d2 to the set, list
//              position), d2 to the set being the minimum over the set's members; e_i = sqrt of that d2
//   chain rank e_i = sqrt(min_{j < i} d2(o_i, o_j)): the points in list order, nothing is selected
//   ac(q) = sum_{i = 1 .. k} w_i e_i, w_i = 2 (k + 1 - i) / (k (k + 1)), float64, i ascending
// The score kernel forms ac(q) k / sum_i ac_ref(o_i), the ceiling kernel fills the degenerate rows in (below).
//
// The chain kernel is outlier_abod.hip's layout with another pair quantity and a selection behind it.  One wave owns one
// item, a workgroup four query rows of one subspace (all four waves walk the same d_s, so the block barriers are uniform).
//   gather   F_s in blocks of kCofFB = 32 features, lanes over (neighbour, feature) feature-fastest (W = 32 features side
//            by side, or the next power of two >= d_s), the loads of block i + 1 issued before the arithmetic of block i
//   stage    the raw values go to LDS as float64 (exact), feature-major [32][KP + 2] per wave, KP = 8 T the padded k; the
//            query's value of the feature sits in the first pad slot (index KP), so the 33rd point costs no re-tiling.
//            Slots of missing neighbours (a >= k, or an index outside the reference set) hold 0 and are never selected.
//            The list itself sits in LDS ([KP] ints per wave), not in registers across the feature loop
//   pairs    lane (I, J) = (lane / 8, lane % 8) owns the T x T block of pairs (T I + i, T J + j) (T = 1, 2, 4 for k <= 8,
//            16, 32): per feature 2 T + 2 doubles from LDS, T^2 subtractions and multiply-adds for the block and one for the
//            query-to-neighbour vector: the lane forms the entry of row T I + J % T, the lanes J < T publish theirs.
//            (a - b)^2 and (b - a)^2 are the same float64, so the matrix is symmetric to the bit
//   matrix   after the feature loop the k x k d2 matrix goes to LDS over the staging buffer ([KP][KP] doubles, 8 KB per
//            wave at KP = 32 against the buffer's 8.5 KB), the query vector next to it
//   chain    lane l < k holds the d2 of point l + 1 to the set.  A step is a wave minimum on the bit pattern (d2 >= 0, so
//            the IEEE bits order like the values), a ballot for the lowest lane that holds it, and one LDS row read that
//            updates every remaining lane; the weighted sum runs wave-uniform in step order.  No atomics anywhere.
#include <float.h>

#include "vgan_common.hpp"

namespace vgan {

constexpr int kCofFB = 32;                       // features per staged block
constexpr int kCofWaves = kBlock / kWave;        // items (query rows) per workgroup

template <int T, bool SBN>
__global__ __launch_bounds__(kBlock, 4) void outlier_cof_chain_kernel(const float* __restrict__ Xq, int ldq, int nq,
                                                                   const float* __restrict__ Xr, int ldr, int nr,
                                                                   const int32_t* __restrict__ feat,
                                                                   const int32_t* __restrict__ feat_off, int first,
                                                                   const int32_t* __restrict__ idx, int k,
                                                                   double* __restrict__ ac_out) {
    constexpr int KP = 8 * T, LD = KP + 2;
    constexpr int NE = KP * kCofFB / kWave;  // staged elements per lane and feature block
    static_assert(KP * KP <= kCofFB * LD, "the d2 matrix reuses the staging buffer");
    __shared__ __attribute__((aligned(16))) double lds_v[kCofWaves][kCofFB * LD];
    __shared__ double lds_q[kCofWaves][KP];
    __shared__ int lds_nb[kCofWaves][KP];

    const int z = blockIdx.y, s = first + z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q_raw = blockIdx.x * kCofWaves + wave;
    const int q = min(q_raw, nq - 1);  // a surplus wave repeats the last row (barriers stay uniform) and stores nothing
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0;
    double* V = lds_v[wave];

    // lanes over (neighbour, feature), feature fastest: W features side by side, 64 / W neighbours per load
    int logw = 5;
    while (logw > 0 && (1 << (logw - 1)) >= ds) --logw;
    const int W = 1 << logw, c = lane & (W - 1), a0 = lane >> logw, astep = kWave >> logw;

    // the reference rows of the list go to LDS (-1 for a missing one: a slot past k, or an index outside the reference set), so
    // that they cost no registers across the feature loop; `valid` keeps one bit per neighbour slot of this lane
    const int32_t* list = idx + ((long)z * nq + q) * k;
    if (lane < KP) {
        const int r = lane < k ? list[lane] : -1;
        lds_nb[wave][lane] = (unsigned)r < (unsigned)nr ? r : -1;
    }
    __syncthreads();
    unsigned valid = 0;
#pragma unroll
    for (int t = 0; t < NE; ++t) {
        const int a = a0 + t * astep;
        if (a < KP && lds_nb[wave][a] >= 0) valid |= 1u << t;
    }
    const float* xq = Xq + (long)q * ldq;

    // every load is unconditional inside a wave-uniform guard (slots past k are skipped by the whole wave); a lane past
    // d_s or on a missing neighbour reads a valid address again and its value is dropped when the block is staged
    float qv = 0.f, rv[NE];
    bool live = false;
#pragma unroll
    for (int t = 0; t < NE; ++t) rv[t] = 0.f;
    const int tload = (k + astep - 1) >> (6 - logw);  // slots t >= tload lie past k for every lane
    auto load_block = [&](int cb) {
        live = cb + c < ds;
        const int f = feat[f0 + min(cb + c, ds - 1)];
        qv = xq[f];
#pragma unroll
        for (int t = 0; t < NE; ++t)
            if (t < tload) rv[t] = Xr[(long)max(lds_nb[wave][min(a0 + t * astep, KP - 1)], 0) * ldr + f];
    };

    double acc[T][T], accq = 0.0;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = 0.0;
    const int I = lane >> 3, J = lane & 7;
    const int aq = T * I + (J & (T - 1));  // the neighbour whose distance to the query this lane forms (lanes J < T publish it)

    load_block(0);
    for (int cb = 0; cb < ds; cb += kCofFB) {
        __syncthreads();  // the pair step of the previous block has read its LDS
        // `valid` is made opaque here: left loop-invariant, its 16 bit tests are hoisted as 16 lane masks and spill SGPRs.
        // A slot past KP (narrow subspaces only) has no bit and writes its 0 to the unused second pad slot
        asm volatile("" : "+v"(valid));
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int a = a0 + t * astep;
            V[c * LD + min(a, KP) + (a >= KP ? 1 : 0)] = (live && (valid >> t & 1u)) ? (double)rv[t] : 0.0;
        }
        if (a0 == 0) V[c * LD + KP] = live ? (double)qv : 0.0;
        __syncthreads();
        if (cb + kCofFB < ds) load_block(cb + kCofFB);
        const int cw = min(kCofFB, ds - cb);
        for (int f = 0; f < cw; ++f) {
            const double* row = V + f * LD;
            double av[T], bv[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                av[i] = row[T * I + i];
                bv[i] = row[T * J + i];
            }
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
    }

    // the d2 matrix over the staging buffer, the query-to-neighbour vector next to it
    __syncthreads();
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) V[(T * I + i) * KP + T * J + j] = acc[i][j];
    if (J < T) lds_q[wave][aq] = accq;
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
    if (lane == 0 && q_raw < nq) ac_out[(long)z * nq + q] = ac;
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

// One workgroup per row s of the score matrix [S, ld] (n scores a row).  A NaN score marks a degenerate row.
//   fit != 0  score_ceiling[s] = the largest score that is not NaN (1 if there is none), n_degenerate[s] = the number of NaNs
//   then every NaN of the row becomes (float)score_ceiling[s].  A maximum and an integer count are order-free.
__global__ __launch_bounds__(kBlock) void outlier_cof_ceiling_kernel(float* __restrict__ score, int ld, int n, int fit,
                                                                     double* __restrict__ score_ceiling,
                                                                     int32_t* __restrict__ n_degenerate) {
    __shared__ float red_m[kBlock / kWave];
    __shared__ int red_c[kBlock / kWave];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* row = score + (long)s * ld;
    float ce;
    if (fit) {
        float m = -INFINITY;
        int cnt = 0;
        for (int i = tid; i < n; i += kBlock) {
            const float v = row[i];
            if (v == v) m = fmaxf(m, v);
            else ++cnt;
        }
        m = wave_max(m);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            red_m[wave] = m;
            red_c[wave] = cnt;
        }
        __syncthreads();
        m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        cnt = red_c[0] + red_c[1] + red_c[2] + red_c[3];
        ce = cnt == n ? 1.f : m;
        if (tid == 0) {
            score_ceiling[s] = (double)ce;
            n_degenerate[s] = cnt;
        }
    } else {
        ce = (float)score_ceiling[s];
    }
    for (int i = tid; i < n; i += kBlock) {
        const float v = row[i];
        if (!(v == v)) row[i] = ce;
    }
}

template <int T>
static void launch_chain(int chain, dim3 grid, hipStream_t st, const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr,
                         const int32_t* feat, const int32_t* feat_off, int first, const int32_t* idx, int k, double* ac_out) {
    if (chain == VGAN_OUTLIER_COF_CHAIN_SBN)
        hipLaunchKernelGGL((outlier_cof_chain_kernel<T, true>), grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off,
                           first, idx, k, ac_out);
    else
        hipLaunchKernelGGL((outlier_cof_chain_kernel<T, false>), grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off,
                           first, idx, k, ac_out);
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
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((nq + kCofWaves - 1) / kCofWaves, count);
    if (k <= 8)
        launch_chain<1>(chain, grid, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k, ac_out);
    else if (k <= 16)
        launch_chain<2>(chain, grid, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k, ac_out);
    else
        launch_chain<4>(chain, grid, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, idx, k, ac_out);
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
    hipLaunchKernelGGL(outlier_cof_ceiling_kernel, dim3(S), dim3(kBlock), 0, (hipStream_t)stream, score, ld, n, fit ? 1 : 0,
                       score_ceiling, n_degenerate);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

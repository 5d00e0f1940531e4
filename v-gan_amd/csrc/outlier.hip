// Outlier scoring over generated subspaces: kNN distance / LOF / Gaussian KDE per subspace, combined with the subspace
// probabilities (the use the reference README names for the learnt subspaces: "ensembling in the Outlier Detection problem").
//
// Per subspace s (feature list F_s, d_s = |F_s|, w_s = round4(d_s)):
//   1. pack     gather F_s of every row into a row-major block [n, w_s] (zero pad), optionally centred, with row norms
//   2. distance a workgroup owns 64 query rows and walks the reference rows 64 at a time (outlier_dist.hpp); the
//               n_q x n_r distance matrix never exists.  Two distance engines feed every consumer:
//                 exact  sum_f (q_f - r_f)^2 on the VALU (small d_s: no cancellation, duplicates give exactly 0)
//                 gram   |q|^2 + |r|^2 - 2 q.r with the fp32 MFMA tile of gemm_core.hpp (large d_s, centred operands)
//               optional split of the reference rows over J workgroups.  Consumers:
//                 knn    top-k on the strict total order (d2, index) + a merge launch: the same k-list for every J and
//                        every chunking; then
//                        refine  recompute the k selected distances in float64 from the raw rows, re-sort by (distance, index)
//                        score   kNN (largest / mean / median of the k distances) or LOF (k_distance, lrd, mean lrd ratio)
//                 kde    pivot sweep (min d2), sum sweep (exp2 terms against the pivot, uint64 fixed point: the same sum
//                        for every J), score (Gaussian -log density in float64)
//   3. combine  out[i] = sum_s p_s score_s[i] in float64, subspaces in order
// Other metrics of knn (vgan_outlier_knn_metric, _pack_unit, _refine_metric): Manhattan, Chebyshev and Minkowski lists come from
// the vector-ALU producer of outlier_metric.hpp on uncentred blocks (ranked by the float32 sum, maximum or sum of p-th powers);
// cosine lists from the Gram engine on rows packed to unit length (d2 = 2 - 2 cos); refine re-measures under the metric.
#include <float.h>
#include <limits.h>

#include "outlier_dist.hpp"
#include "outlier_metric.hpp"

namespace vgan {

// k best (d2, index) pairs of one thread, ascending; unused slots hold (+inf, INT_MAX)
template <int K>
struct TopK {
    float d[K];
    int i[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            d[t] = INFINITY;
            i[t] = INT_MAX;
        }
    }
    __device__ __forceinline__ void push(float nd, int ni) {
        if (!cand_less(nd, ni, d[K - 1], i[K - 1])) return;  // prune against the current K-th
#pragma unroll
        for (int t = K - 1; t > 0; --t) {
            const bool up = cand_less(nd, ni, d[t - 1], i[t - 1]);
            const bool here = cand_less(nd, ni, d[t], i[t]);
            d[t] = up ? d[t - 1] : (here ? nd : d[t]);
            i[t] = up ? i[t - 1] : (here ? ni : i[t]);
        }
        if (cand_less(nd, ni, d[0], i[0])) {
            d[0] = nd;
            i[0] = ni;
        }
    }
};

// LDS of the knn kernel: the engine's images, reused by the final merge of the four waves' lists
template <int K, bool GRAM>
struct KnnLds {
    static constexpr int kEngine = DistLds<GRAM>::kFloats;
    static constexpr int kMerge = 2 * 2 * K * kOTile;  // (d, i) of two waves
    static constexpr int kFloats = kEngine > kMerge ? kEngine : kMerge;
};

// kNN selection over the distance producer.  Lane l of every wave owns query row q0 + l; wave w selects among columns
// [16w, 16w + 16) of each 64-row reference tile, then the four lists of a row are merged.
template <int K, bool GRAM>
__global__ __launch_bounds__(kBlock, 2) void outlier_knn_kernel(const float* __restrict__ Pq, const float* __restrict__ sqq, int nq,
                                                                const float* __restrict__ Pr, const float* __restrict__ sqr, int nr,
                                                                const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                                int first, int k, int exclude_self, int splits,
                                                                float* __restrict__ part_d, int32_t* __restrict__ part_i,
                                                                int32_t* __restrict__ nbr) {
    __shared__ __attribute__((aligned(16))) float lds[KnnLds<K, GRAM>::kFloats];
    const int z = blockIdx.z, slice = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x * kOTile + lane;

    TopK<K> top;
    top.init();
    outlier_distances<GRAM>(Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, lds, [&](const float (&d2)[16], int c0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j;
            if (c < nr && !(exclude_self && c == q)) top.push(d2[j], c);
        }
    });

    // merge the four waves' lists of each row: waves 2, 3 hand theirs to waves 0, 1, then wave 1 to wave 0
    __syncthreads();
    float* md = lds;
    int* mi = reinterpret_cast<int*>(lds + 2 * K * kOTile);
    for (int round = 0; round < 2; ++round) {
        const int hi = round == 0 ? 2 : 1;  // waves [hi, 2 hi) give, waves [0, hi) take
        if (wave >= hi && wave < 2 * hi) {
#pragma unroll
            for (int t = 0; t < K; ++t) {
                md[((wave - hi) * K + t) * kOTile + lane] = top.d[t];
                mi[((wave - hi) * K + t) * kOTile + lane] = top.i[t];
            }
        }
        __syncthreads();
        if (wave < hi) {
#pragma unroll
            for (int t = 0; t < K; ++t) top.push(md[(wave * K + t) * kOTile + lane], mi[(wave * K + t) * kOTile + lane]);
        }
        __syncthreads();
    }
    if (wave == 0 && q < nq) {
        if (splits == 1) {
            int32_t* o = nbr + ((long)z * nq + q) * k;
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t < k) o[t] = top.i[t];
        } else {
            const long off = (((long)z * splits + slice) * nq + q) * k;
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t < k) {
                    part_d[off + t] = top.d[t];
                    part_i[off + t] = top.i[t];
                }
        }
    }
}

// The tail of outlier_knn_kernel as a routine, for the metric kernel below: merges the four waves' lists of each row through lds
// (KnnLds::kMerge floats, the producer done with it) and stores the k-list of row q, or the slice's list when the reference rows
// are split.  outlier_knn_kernel keeps its tail spelt out: routed through this routine the compiler allocates its registers
// differently (K = 8, exact engine: 126 VGPRs against 84), and its device code is to stay the one that was measured.
template <int K>
__device__ __forceinline__ void knn_merge_store(TopK<K>& top, float* lds, int q, int nq, int k, int splits, float* __restrict__ part_d,
                                                int32_t* __restrict__ part_i, int32_t* __restrict__ nbr) {
    const int z = blockIdx.z, slice = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    float* md = lds;
    int* mi = reinterpret_cast<int*>(lds + 2 * K * kOTile);
    for (int round = 0; round < 2; ++round) {
        const int hi = round == 0 ? 2 : 1;  // waves [hi, 2 hi) give, waves [0, hi) take
        if (wave >= hi && wave < 2 * hi) {
#pragma unroll
            for (int t = 0; t < K; ++t) {
                md[((wave - hi) * K + t) * kOTile + lane] = top.d[t];
                mi[((wave - hi) * K + t) * kOTile + lane] = top.i[t];
            }
        }
        __syncthreads();
        if (wave < hi) {
#pragma unroll
            for (int t = 0; t < K; ++t) top.push(md[(wave * K + t) * kOTile + lane], mi[(wave * K + t) * kOTile + lane]);
        }
        __syncthreads();
    }
    if (wave == 0 && q < nq) {
        if (splits == 1) {
            int32_t* o = nbr + ((long)z * nq + q) * k;
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t < k) o[t] = top.i[t];
        } else {
            const long off = (((long)z * splits + slice) * nq + q) * k;
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t < k) {
                    part_d[off + t] = top.d[t];
                    part_i[off + t] = top.i[t];
                }
        }
    }
}

// The same selection over the Minkowski-family producer (outlier_metric.hpp); the candidates are ranked by (g, index)
template <int K, class Term>
__global__ __launch_bounds__(kBlock, 2) void outlier_knn_metric_kernel(const float* __restrict__ Pq, int nq, const float* __restrict__ Pr,
                                                                       int nr, const int32_t* __restrict__ feat_off,
                                                                       const int64_t* __restrict__ col_off, int first, int k,
                                                                       int exclude_self, int splits, Term term, float* __restrict__ part_d,
                                                                       int32_t* __restrict__ part_i, int32_t* __restrict__ nbr) {
    constexpr int kMerge = 2 * 2 * K * kOTile;
    __shared__ __attribute__((aligned(16))) float lds[kMetricLdsFloats > kMerge ? kMetricLdsFloats : kMerge];
    const int q = blockIdx.x * kOTile + (threadIdx.x & 63);

    TopK<K> top;
    top.init();
    outlier_metric_distances(Pq, nq, Pr, nr, feat_off, col_off, first, splits, term, lds, [&](const float (&g)[16], int c0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j;
            if (c < nr && !(exclude_self && c == q)) top.push(g[j], c);
        }
    });

    knn_merge_store<K>(top, lds, q, nq, k, splits, part_d, part_i, nbr);
}

// the J partial lists of a (subspace, query row) -> its k-list; one thread per row
template <int K>
__global__ void outlier_knn_merge_kernel(const float* __restrict__ part_d, const int32_t* __restrict__ part_i, int nq, int count,
                                         int k, int splits, int32_t* __restrict__ nbr) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (long)count * nq) return;
    const long z = row / nq, q = row % nq;
    TopK<K> top;
    top.init();
    for (int j = 0; j < splits; ++j) {
        const long off = ((z * splits + j) * nq + q) * k;
        for (int t = 0; t < k; ++t) top.push(part_d[off + t], part_i[off + t]);
    }
    int32_t* o = nbr + row * k;
#pragma unroll
    for (int t = 0; t < K; ++t)
        if (t < k) o[t] = top.i[t];
}

// c_s = log2(e) / (2 h^2) in float32, finite (a kernel term is exp2f(c_s (m_q - d2)) = exp(-(d2 - m_q) / (2 h^2)));
// the sum sweep and the score take the same value, so the score is exact for the bandwidth c_s stands for
__device__ __forceinline__ float kde_coef(double h) { return fminf((float)(1.4426950408889634 / (2.0 * h * h)), FLT_MAX); }

// pivot[row] = +inf bits, acc[row] = 0 for the count * nq rows of a kde call
__global__ void outlier_kde_init_kernel(unsigned* __restrict__ pivot, unsigned long long* __restrict__ acc, long rows) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    pivot[row] = 0x7f800000u;
    acc[row] = 0ull;
}

// The two Gaussian-KDE sweeps over the distance producer; a row is (chunk subspace z, query q), at z * nq + q.
//   PIVOT  m_q = min of d2 over the summed reference rows -> atomicMin into pivot (float bits as unsigned: d2 >= 0, so
//          the bit order is the value order; -0 is mapped to +0).  Min is exact: the same m_q for every J.
//   !PIVOT sum_r exp2f(c_s (m_q - d2)): every term <= 1 and the nearest row gives exactly 1.  A lane sums its 16 columns of
//          a tile in float32 in fixed order and adds the partial, rounded at 2^-40, to a uint64 fixed-point accumulator;
//          the merge and the atomicAdd into acc are outlier_dist.hpp's fixed_point_row_sums.  Integer sums are associative:
//          the same acc for every J.  Terms <= 1 and nr < 2^23 keep acc below 2^63.
// One atomic per (slice, row), from wave 0, whose 64 lanes hold 64 consecutive rows.
template <bool GRAM, bool PIVOT>
__global__ __launch_bounds__(kBlock, 2) void outlier_kde_kernel(const float* __restrict__ Pq, const float* __restrict__ sqq, int nq,
                                                                const float* __restrict__ Pr, const float* __restrict__ sqr, int nr,
                                                                const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                                int first, int exclude_self, int splits, const double* __restrict__ bandwidth,
                                                                unsigned* __restrict__ pivot, unsigned long long* __restrict__ acc) {
    __shared__ __attribute__((aligned(16))) float lds[DistLds<GRAM>::kFloats];
    const int z = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x * kOTile + lane;
    const long row = (long)z * nq + q;
    if constexpr (PIVOT) {
        static_assert(DistLds<GRAM>::kFloats >= kBlock, "merge scratch");
        float m = INFINITY;
        outlier_distances<GRAM>(Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, lds, [&](const float (&d2)[16], int c0) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = c0 + j;
                if (c < nr && !(exclude_self && c == q)) m = fminf(m, d2[j]);
            }
        });
        __syncthreads();
        lds[tid] = m;
        __syncthreads();
        if (wave == 0 && q < nq) {
            m = fminf(fminf(lds[lane], lds[kWave + lane]), fminf(lds[2 * kWave + lane], lds[3 * kWave + lane]));
            atomicMin(pivot + row, __float_as_uint(m) & 0x7fffffffu);
        }
    } else {
        const float c_s = kde_coef(bandwidth[first + z]);
        const float m = q < nq ? __uint_as_float(pivot[row]) : 0.f;
        fixed_point_row_sums<GRAM>(Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, lds, acc, [&](const float (&d2)[16], int c0) {
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = c0 + j;
                if (c < nr && !(exclude_self && c == q)) t += exp2f(c_s * (m - d2[j]));
            }
            return (unsigned long long)rintf(t * 0x1p40f);
        });
    }
}

// score[score_row[z], q] = -log p_s(q) = -(ln(acc 2^-40) - c_s m_q ln 2 - ln n_sum - d_s ln h - d_s / 2 ln 2 pi), float64;
// one thread per row
__global__ void outlier_kde_score_kernel(const unsigned* __restrict__ pivot, const unsigned long long* __restrict__ acc, int nq,
                                         int count, const int32_t* __restrict__ feat_off, int first, const double* __restrict__ bandwidth,
                                         int n_sum, float* __restrict__ score, const int32_t* __restrict__ score_row, int ld_score) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (long)count * nq) return;
    const int z = (int)(row / nq), q = (int)(row % nq), s = first + z;
    const int ds = feat_off[s + 1] - feat_off[s];
    const double h = bandwidth[s];
    const double m = __uint_as_float(pivot[row]);
    const double lp = log((double)acc[row] * 0x1p-40) - (double)kde_coef(h) * m * 0.6931471805599453 - log((double)n_sum) -
                      ds * log(h) - 0.5 * ds * 1.8378770664093453;  // ln(2 pi)
    score[(long)(score_row ? score_row[z] : z) * ld_score + q] = (float)(-lp);
}

// packed[n * (col_off[s] - col_off[first]) + i * w_s + c] = X[i, feat[feat_off[s] + c]] - center[...] (0 for c >= d_s);
// sq[(s - first) * n + i] = its squared norm.  Grid (row blocks of 64, subspaces); one wave per row, lanes over features.
__global__ void outlier_pack_kernel(const float* __restrict__ X, int ldx, int n, const float* __restrict__ center,
                                    const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                    const int64_t* __restrict__ col_off, int first, float* __restrict__ packed, float* __restrict__ sq) {
    const int z = blockIdx.y, s = first + z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0, w = (ds + 3) & ~3;
    float* P = packed + (col_off[s] - col_off[first]) * n;
    for (int i = blockIdx.x * kOTile + wave; i < min(n, (blockIdx.x + 1) * kOTile); i += kBlock / kWave) {
        float acc = 0.f;
        for (int c = lane; c < w; c += kWave) {
            float v = 0.f;
            if (c < ds) {
                const int f = feat[f0 + c];
                v = X[(long)i * ldx + f];
                if (center != nullptr) v -= center[f];
            }
            P[(long)i * w + c] = v;
            acc = fmaf(v, v, acc);
        }
        acc = wave_sum(acc);
        if (sq != nullptr && lane == 0) sq[(long)z * n + i] = acc;
    }
}

// One wave per (subspace, query row): lane t < k recomputes |x_q - x_{nbr_t}| over F_s in float64 from the raw rows, then the
// k values are ranked by (distance as float32, index) and written in that order.  kdist (may be NULL) gets the k-th.
__global__ void outlier_refine_kernel(const float* __restrict__ Xq, int ldq, int nq, const float* __restrict__ Xr, int ldr, int nr,
                                      const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off, int first, int count,
                                      const int32_t* __restrict__ nbr, int k, int32_t* __restrict__ out_idx,
                                      float* __restrict__ out_dist, float* __restrict__ kdist) {
    const long row = (long)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (row >= (long)count * nq) return;
    const int lane = threadIdx.x & 63;
    const int z = (int)(row / nq), q = (int)(row % nq), s = first + z;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0;
    int idx = INT_MAX;
    float dist = INFINITY;
    if (lane < k) idx = nbr[row * k + lane];
    if (idx >= 0 && idx < nr) {
        const float* xq = Xq + (long)q * ldq;
        const float* xr = Xr + (long)idx * ldr;
        double acc = 0.0;
        for (int c = 0; c < ds; ++c) {
            const int f = feat[f0 + c];
            const double e = (double)xq[f] - (double)xr[f];
            acc = fma(e, e, acc);
        }
        dist = (float)sqrt(acc);
    }
    int rank = 0;
    for (int u = 0; u < k; ++u) {
        const float du = __shfl(dist, u, 64);
        const int iu = __shfl(idx, u, 64);
        rank += cand_less(du, iu, dist, idx) ? 1 : 0;
    }
    if (lane < k) {
        out_idx[row * k + rank] = idx;
        out_dist[row * k + rank] = dist;
        if (kdist != nullptr && rank == k - 1) kdist[row] = dist;
    }
}

// outlier_pack_kernel without a centre, every row scaled to unit length: packed[...] = (float)(X[i, f] / |X[i, F_s]|), the norm
// and the quotient in float64 (a zero row stays zero); sq = 1 for every row, so that the Gram engine's d2 is 2 - 2 cos and a
// zero row lies at d2 = 2 (cosine distance 1) from every row.
__global__ void outlier_pack_unit_kernel(const float* __restrict__ X, int ldx, int n, const int32_t* __restrict__ feat,
                                         const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off, int first,
                                         float* __restrict__ packed, float* __restrict__ sq) {
    const int z = blockIdx.y, s = first + z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0, w = (ds + 3) & ~3;
    float* P = packed + (col_off[s] - col_off[first]) * n;
    for (int i = blockIdx.x * kOTile + wave; i < min(n, (blockIdx.x + 1) * kOTile); i += kBlock / kWave) {
        double acc = 0.0;
        for (int c = lane; c < ds; c += kWave) {
            const double v = X[(long)i * ldx + feat[f0 + c]];
            acc = fma(v, v, acc);
        }
        acc = wave_sum(acc);
        const double scale = acc > 0.0 ? 1.0 / sqrt(acc) : 0.0;
        for (int c = lane; c < w; c += kWave) P[(long)i * w + c] = c < ds ? (float)((double)X[(long)i * ldx + feat[f0 + c]] * scale) : 0.f;
        if (sq != nullptr && lane == 0) sq[(long)z * n + i] = 1.f;
    }
}

// outlier_refine_kernel under another metric (METRIC: VGAN_OUTLIER_METRIC_*), float64 from the raw rows, features ascending:
// sum |e|, max |e|, (sum |e|^p)^(1 / p), or 1 - <x, y> / (|x| |y|) clipped to [0, 2] (exactly 1 when a norm is 0)
template <int METRIC>
__global__ void outlier_refine_metric_kernel(const float* __restrict__ Xq, int ldq, int nq, const float* __restrict__ Xr, int ldr, int nr,
                                             const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off, int first,
                                             int count, const int32_t* __restrict__ nbr, int k, double p, int32_t* __restrict__ out_idx,
                                             float* __restrict__ out_dist, float* __restrict__ kdist) {
    const long row = (long)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (row >= (long)count * nq) return;
    const int lane = threadIdx.x & 63;
    const int z = (int)(row / nq), q = (int)(row % nq), s = first + z;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0;
    int idx = INT_MAX;
    float dist = INFINITY;
    if (lane < k) idx = nbr[row * k + lane];
    if (idx >= 0 && idx < nr) {
        const float* xq = Xq + (long)q * ldq;
        const float* xr = Xr + (long)idx * ldr;
        double acc = 0.0, nx = 0.0, ny = 0.0;
        for (int c = 0; c < ds; ++c) {
            const int f = feat[f0 + c];
            const double x = xq[f], y = xr[f], e = fabs(x - y);
            if constexpr (METRIC == VGAN_OUTLIER_METRIC_MANHATTAN) acc += e;
            if constexpr (METRIC == VGAN_OUTLIER_METRIC_CHEBYSHEV) acc = fmax(acc, e);
            if constexpr (METRIC == VGAN_OUTLIER_METRIC_MINKOWSKI) acc += pow(e, p);
            if constexpr (METRIC == VGAN_OUTLIER_METRIC_COSINE) {
                acc = fma(x, y, acc);
                nx = fma(x, x, nx);
                ny = fma(y, y, ny);
            }
        }
        if constexpr (METRIC == VGAN_OUTLIER_METRIC_MINKOWSKI) acc = pow(acc, 1.0 / p);
        if constexpr (METRIC == VGAN_OUTLIER_METRIC_COSINE)
            acc = (nx > 0.0 && ny > 0.0) ? fmin(fmax(1.0 - acc / (sqrt(nx) * sqrt(ny)), 0.0), 2.0) : 1.0;
        dist = (float)acc;
    }
    int rank = 0;
    for (int u = 0; u < k; ++u) {
        const float du = __shfl(dist, u, 64);
        const int iu = __shfl(idx, u, 64);
        rank += cand_less(du, iu, dist, idx) ? 1 : 0;
    }
    if (lane < k) {
        out_idx[row * k + rank] = idx;
        out_dist[row * k + rank] = dist;
        if (kdist != nullptr && rank == k - 1) kdist[row] = dist;
    }
}

// One thread per (subspace, query row) over its sorted list (dist, idx).
//   method 0/1/2: kNN largest / mean / median -> score
//   method 3:     lrd(p) = 1 / (mean_o max(kdist_ref(o), d(p, o)) + 1e-10) -> lrd_out
//   method 4:     LOF(p) = mean_o lrd_ref(o) / lrd(p)                          -> score
// score row of subspace z: score_row[z] (score_row may be NULL: row z), leading dimension ld_score.
__global__ void outlier_score_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist, int nq, int k, int count,
                                     int method, const float* __restrict__ kdist_ref, const double* __restrict__ lrd_ref, int nr,
                                     float* __restrict__ score, const int32_t* __restrict__ score_row, int ld_score,
                                     double* __restrict__ lrd_out) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (long)count * nq) return;
    const int z = (int)(row / nq), q = (int)(row % nq);
    const float* d = dist + row * k;
    const int32_t* o = idx + row * k;
    double v;
    if (method == VGAN_OUTLIER_KNN_LARGEST) {
        v = d[k - 1];
    } else if (method == VGAN_OUTLIER_KNN_MEAN) {
        double a = 0.0;
        for (int t = 0; t < k; ++t) a += d[t];
        v = a / k;
    } else if (method == VGAN_OUTLIER_KNN_MEDIAN) {
        v = (k & 1) ? (double)d[k / 2] : 0.5 * ((double)d[k / 2 - 1] + (double)d[k / 2]);
    } else {
        for (int t = 0; t < k; ++t)
            if ((unsigned)o[t] >= (unsigned)nr) return;  // not a list of refine: nothing to read
        const float* kd = kdist_ref + (long)z * nr;
        double a = 0.0;
        for (int t = 0; t < k; ++t) a += fmax((double)kd[o[t]], (double)d[t]);
        const double lrd = 1.0 / (a / k + 1e-10);
        if (method == VGAN_OUTLIER_LRD) {
            lrd_out[row] = lrd;
            return;
        }
        const double* lr = lrd_ref + (long)z * nr;
        double b = 0.0;
        for (int t = 0; t < k; ++t) b += lr[o[t]] / lrd;
        v = b / k;
    }
    score[(long)(score_row ? score_row[z] : z) * ld_score + q] = (float)v;
}

// out[i] = sum_s p[s] * score[s, i], float64, s ascending
__global__ void outlier_combine_kernel(const float* __restrict__ score, int ld, int S, int n, const double* __restrict__ p,
                                       double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += p[s] * (double)score[(long)s * ld + i];
    out[i] = a;
}

template <int K>
static int launch_knn(const float* Pq, const float* sqq, int nq, const float* Pr, const float* sqr, int nr, const int32_t* feat_off,
                      const int64_t* col_off, int first, int count, int k, int exclude_self, int engine, int splits, float* part_d,
                      int32_t* part_i, int32_t* nbr, hipStream_t st) {
    dispatch_engine(engine, [&](auto gram) {
        hipLaunchKernelGGL((outlier_knn_kernel<K, decltype(gram)::value>), dist_grid(nq, splits, count), dim3(kBlock), 0, st, Pq, sqq, nq, Pr,
                           sqr, nr, feat_off, col_off, first, k, exclude_self, splits, part_d, part_i, nbr);
    });
    VGAN_CHECK_LAUNCH();
    if (splits > 1) {
        const long rows = (long)count * nq;
        hipLaunchKernelGGL(outlier_knn_merge_kernel<K>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, part_d, part_i, nq,
                           count, k, splits, nbr);
        VGAN_CHECK_LAUNCH();
    }
    return VGAN_OK;
}

template <int K, class Term>
static int launch_knn_metric(const float* Pq, int nq, const float* Pr, int nr, const int32_t* feat_off, const int64_t* col_off, int first,
                             int count, int k, int exclude_self, Term term, int splits, float* part_d, int32_t* part_i, int32_t* nbr,
                             hipStream_t st) {
    hipLaunchKernelGGL((outlier_knn_metric_kernel<K, Term>), dist_grid(nq, splits, count), dim3(kBlock), 0, st, Pq, nq, Pr, nr, feat_off,
                       col_off, first, k, exclude_self, splits, term, part_d, part_i, nbr);
    VGAN_CHECK_LAUNCH();
    if (splits > 1) {
        const long rows = (long)count * nq;
        hipLaunchKernelGGL(outlier_knn_merge_kernel<K>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, part_d, part_i, nq,
                           count, k, splits, nbr);
        VGAN_CHECK_LAUNCH();
    }
    return VGAN_OK;
}

template <class Term>
static int launch_knn_metric_k(const float* Pq, int nq, const float* Pr, int nr, const int32_t* feat_off, const int64_t* col_off,
                               int first, int count, int k, int exclude_self, Term term, int splits, float* part_d, int32_t* part_i,
                               int32_t* nbr, hipStream_t st) {
    if (k <= 8) return launch_knn_metric<8>(Pq, nq, Pr, nr, feat_off, col_off, first, count, k, exclude_self, term, splits, part_d, part_i, nbr, st);
    if (k <= 16) return launch_knn_metric<16>(Pq, nq, Pr, nr, feat_off, col_off, first, count, k, exclude_self, term, splits, part_d, part_i, nbr, st);
    return launch_knn_metric<32>(Pq, nq, Pr, nr, feat_off, col_off, first, count, k, exclude_self, term, splits, part_d, part_i, nbr, st);
}

// p of VGAN_OUTLIER_METRIC_MINKOWSKI: finite, in (0, 8]
static bool minkowski_p_ok(double p) { return p > 0.0 && p <= VGAN_OUTLIER_MAX_P; }  // false for NaN

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_outlier_pack(const float* X, int ldx, int n, int d, const float* center, const int32_t* feat,
                                 const int32_t* feat_off, const int64_t* col_off, int first, int count, float* packed, float* sq,
                                 vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && feat && feat_off && col_off && packed && n > 0 && d > 0 && ldx >= d && first >= 0 && count > 0);
    VGAN_CHECK_ARG(count <= 65535 && aligned16(packed));
    hipLaunchKernelGGL(outlier_pack_kernel, dim3((n + kOTile - 1) / kOTile, count), dim3(kBlock), 0, (hipStream_t)stream, X, ldx, n,
                       center, feat, feat_off, col_off, first, packed, sq);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_knn(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                                const int32_t* feat_off, const int64_t* col_off, int first, int count, int k, int exclude_self,
                                int engine, int splits, float* part_d, int32_t* part_i, int32_t* nbr, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Pq && Pr && feat_off && col_off && nbr && nq > 0 && nr > 0 && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(k >= 1 && k <= VGAN_OUTLIER_MAX_K);
    VGAN_CHECK_ARG(nr >= k + (exclude_self ? 1 : 0) && (!exclude_self || nq == nr));
    VGAN_CHECK_ARG(dist_args_ok(engine, sq_q && sq_r, splits, Pq, Pr) && (splits == 1 || (part_d && part_i)));
    const hipStream_t st = (hipStream_t)stream;
    if (k <= 8) return launch_knn<8>(Pq, sq_q, nq, Pr, sq_r, nr, feat_off, col_off, first, count, k, exclude_self, engine, splits, part_d, part_i, nbr, st);
    if (k <= 16) return launch_knn<16>(Pq, sq_q, nq, Pr, sq_r, nr, feat_off, col_off, first, count, k, exclude_self, engine, splits, part_d, part_i, nbr, st);
    return launch_knn<32>(Pq, sq_q, nq, Pr, sq_r, nr, feat_off, col_off, first, count, k, exclude_self, engine, splits, part_d, part_i, nbr, st);
}

extern "C" int vgan_outlier_pack_unit(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off,
                                      const int64_t* col_off, int first, int count, float* packed, float* sq, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && feat && feat_off && col_off && packed && n > 0 && d > 0 && ldx >= d && first >= 0 && count > 0);
    VGAN_CHECK_ARG(count <= 65535 && aligned16(packed));
    hipLaunchKernelGGL(outlier_pack_unit_kernel, dim3((n + kOTile - 1) / kOTile, count), dim3(kBlock), 0, (hipStream_t)stream, X, ldx, n,
                       feat, feat_off, col_off, first, packed, sq);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_knn_metric(const float* Pq, int nq, const float* Pr, int nr, const int32_t* feat_off, const int64_t* col_off,
                                       int first, int count, int k, int exclude_self, int metric, double p, int splits, float* part_d,
                                       int32_t* part_i, int32_t* nbr, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Pq && Pr && feat_off && col_off && nbr && nq > 0 && nr > 0 && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(k >= 1 && k <= VGAN_OUTLIER_MAX_K);
    VGAN_CHECK_ARG(nr >= k + (exclude_self ? 1 : 0) && (!exclude_self || nq == nr));
    VGAN_CHECK_ARG(metric == VGAN_OUTLIER_METRIC_MANHATTAN || metric == VGAN_OUTLIER_METRIC_CHEBYSHEV ||
                   metric == VGAN_OUTLIER_METRIC_MINKOWSKI);
    VGAN_CHECK_ARG(metric != VGAN_OUTLIER_METRIC_MINKOWSKI || minkowski_p_ok(p));
    VGAN_CHECK_ARG(dist_args_ok(VGAN_OUTLIER_ENGINE_EXACT, false, splits, Pq, Pr) && (splits == 1 || (part_d && part_i)));
    const hipStream_t st = (hipStream_t)stream;
    if (metric == VGAN_OUTLIER_METRIC_CHEBYSHEV)
        return launch_knn_metric_k(Pq, nq, Pr, nr, feat_off, col_off, first, count, k, exclude_self, MetricLinf{}, splits, part_d, part_i, nbr, st);
    if (metric == VGAN_OUTLIER_METRIC_MANHATTAN || p == 1.0)  // p == 1 is the Manhattan path
        return launch_knn_metric_k(Pq, nq, Pr, nr, feat_off, col_off, first, count, k, exclude_self, MetricL1{}, splits, part_d, part_i, nbr, st);
    return launch_knn_metric_k(Pq, nq, Pr, nr, feat_off, col_off, first, count, k, exclude_self, MetricLp{(float)p}, splits, part_d, part_i, nbr, st);
}

extern "C" int vgan_outlier_kde(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                                const int32_t* feat_off, const int64_t* col_off, int first, int count, const double* bandwidth,
                                int exclude_self, int engine, int splits, uint32_t* pivot, uint64_t* acc, float* score,
                                const int32_t* score_row, int ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Pq && Pr && feat_off && col_off && bandwidth && pivot && acc && score && nq > 0 && nr > 0 && first >= 0);
    VGAN_CHECK_ARG(count > 0 && count <= 65535 && ld_score >= nq && nr <= VGAN_OUTLIER_KDE_MAX_ROWS);
    VGAN_CHECK_ARG(!exclude_self || (nq == nr && nr >= 2));
    VGAN_CHECK_ARG(dist_args_ok(engine, sq_q && sq_r, splits, Pq, Pr));
    const hipStream_t st = (hipStream_t)stream;
    const long rows = (long)count * nq;
    unsigned* piv = reinterpret_cast<unsigned*>(pivot);
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(acc);
    hipLaunchKernelGGL(outlier_kde_init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, piv, sum, rows);
    VGAN_CHECK_LAUNCH();
    dispatch_engine(engine, [&](auto gram) {  // the pivot sweep, then the sum sweep
        hipLaunchKernelGGL((outlier_kde_kernel<decltype(gram)::value, true>), dist_grid(nq, splits, count), dim3(kBlock), 0, st, Pq, sq_q, nq,
                           Pr, sq_r, nr, feat_off, col_off, first, exclude_self, splits, bandwidth, piv, sum);
        hipLaunchKernelGGL((outlier_kde_kernel<decltype(gram)::value, false>), dist_grid(nq, splits, count), dim3(kBlock), 0, st, Pq, sq_q, nq,
                           Pr, sq_r, nr, feat_off, col_off, first, exclude_self, splits, bandwidth, piv, sum);
    });
    VGAN_CHECK_LAUNCH();
    hipLaunchKernelGGL(outlier_kde_score_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, piv, sum, nq, count, feat_off,
                       first, bandwidth, exclude_self ? nr - 1 : nr, score, score_row, ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_refine(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                                   const int32_t* feat_off, int first, int count, const int32_t* nbr, int k, int32_t* out_idx,
                                   float* out_dist, float* kdist, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && Xr && feat && feat_off && nbr && out_idx && out_dist && nq > 0 && nr > 0 && d > 0);
    VGAN_CHECK_ARG(ldq >= d && ldr >= d && first >= 0 && count > 0 && k >= 1 && k <= VGAN_OUTLIER_MAX_K && nr >= k);
    const long rows = (long)count * nq;
    hipLaunchKernelGGL(outlier_refine_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(kBlock), 0, (hipStream_t)stream, Xq, ldq, nq, Xr, ldr,
                       nr, feat, feat_off, first, count, nbr, k, out_idx, out_dist, kdist);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_refine_metric(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                                          const int32_t* feat_off, int first, int count, const int32_t* nbr, int k, int metric, double p,
                                          int32_t* out_idx, float* out_dist, float* kdist, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && Xr && feat && feat_off && nbr && out_idx && out_dist && nq > 0 && nr > 0 && d > 0);
    VGAN_CHECK_ARG(ldq >= d && ldr >= d && first >= 0 && count > 0 && k >= 1 && k <= VGAN_OUTLIER_MAX_K && nr >= k);
    VGAN_CHECK_ARG(metric >= VGAN_OUTLIER_METRIC_EUCLIDEAN && metric <= VGAN_OUTLIER_METRIC_COSINE);
    VGAN_CHECK_ARG(metric != VGAN_OUTLIER_METRIC_MINKOWSKI || minkowski_p_ok(p));
    if (metric == VGAN_OUTLIER_METRIC_MINKOWSKI && p == 2.0) metric = VGAN_OUTLIER_METRIC_EUCLIDEAN;  // the Euclidean path
    if (metric == VGAN_OUTLIER_METRIC_MINKOWSKI && p == 1.0) metric = VGAN_OUTLIER_METRIC_MANHATTAN;  // the Manhattan path
    const long rows = (long)count * nq;
    const dim3 grid((unsigned)((rows + 3) / 4));
    const hipStream_t st = (hipStream_t)stream;
    if (metric == VGAN_OUTLIER_METRIC_EUCLIDEAN)
        hipLaunchKernelGGL(outlier_refine_kernel, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, count, nbr, k,
                           out_idx, out_dist, kdist);
    else if (metric == VGAN_OUTLIER_METRIC_MANHATTAN)
        hipLaunchKernelGGL(outlier_refine_metric_kernel<VGAN_OUTLIER_METRIC_MANHATTAN>, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr,
                           feat, feat_off, first, count, nbr, k, p, out_idx, out_dist, kdist);
    else if (metric == VGAN_OUTLIER_METRIC_CHEBYSHEV)
        hipLaunchKernelGGL(outlier_refine_metric_kernel<VGAN_OUTLIER_METRIC_CHEBYSHEV>, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr,
                           feat, feat_off, first, count, nbr, k, p, out_idx, out_dist, kdist);
    else if (metric == VGAN_OUTLIER_METRIC_MINKOWSKI)
        hipLaunchKernelGGL(outlier_refine_metric_kernel<VGAN_OUTLIER_METRIC_MINKOWSKI>, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr,
                           feat, feat_off, first, count, nbr, k, p, out_idx, out_dist, kdist);
    else
        hipLaunchKernelGGL(outlier_refine_metric_kernel<VGAN_OUTLIER_METRIC_COSINE>, grid, dim3(kBlock), 0, st, Xq, ldq, nq, Xr, ldr, nr,
                           feat, feat_off, first, count, nbr, k, p, out_idx, out_dist, kdist);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_score(const int32_t* idx, const float* dist, int nq, int k, int count, int method, const float* kdist_ref,
                                  const double* lrd_ref, int nr, float* score, const int32_t* score_row, int ld_score, double* lrd_out,
                                  vgan_stream_t stream) {
    VGAN_CHECK_ARG(idx && dist && nq > 0 && count > 0 && k >= 1 && k <= VGAN_OUTLIER_MAX_K);
    VGAN_CHECK_ARG(method >= VGAN_OUTLIER_KNN_LARGEST && method <= VGAN_OUTLIER_LOF);
    VGAN_CHECK_ARG(method < VGAN_OUTLIER_LRD || (kdist_ref && nr >= k));
    VGAN_CHECK_ARG(method == VGAN_OUTLIER_LRD ? lrd_out != nullptr : (score != nullptr && ld_score >= nq));
    VGAN_CHECK_ARG(method != VGAN_OUTLIER_LOF || lrd_ref);
    const long rows = (long)count * nq;
    hipLaunchKernelGGL(outlier_score_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, dist, nq, k,
                       count, method, kdist_ref, lrd_ref, nr, score, score_row, ld_score, lrd_out);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_outlier_combine(const float* score, int ld, int S, int n, const double* weights, double* out,
                                    vgan_stream_t stream) {
    VGAN_CHECK_ARG(score && weights && out && S > 0 && n > 0 && ld >= n);
    hipLaunchKernelGGL(outlier_combine_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, score, ld, S, n, weights, out);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

// Batched k-means (Lloyd) over generated subspaces and the cluster-based local outlier factor on top of it
// (v-gan_amd/outlier.py: SubspaceCBLOF).  C <= 64 clusters, so the centres of a subspace are one 64-row reference tile of
// the distance producer of outlier_dist.hpp.
//
// Per chunk of subspaces, packed once (vgan_outlier_pack), one Lloyd iteration is three launches:
//   assign   a third consumer of outlier_distances: arg-min on (d2, centre index) over the <= 64 centre columns, the four
//            waves merged through LDS; writes the labels and adds the number of changed labels of the subspace (integer).
//   partial  float64 sums per (cluster, feature) over a fixed partition of the rows (slices of kCSlice rows, which depends
//            on n alone), from the raw float32 rows.  A thread owns one feature column of a row group and keeps its C
//            accumulators in LDS (column [c][thread]: no two threads share one, so no atomics); the row groups are added
//            in order.  Column d_s of a subspace is the constant 1: its sums are the cluster sizes, exact integers.
//   final    one workgroup per subspace adds the slice partials in order, divides, takes the squared centre shift in a
//            fixed tree, rewrites the float32 operand image and its norms and sets the subspace's done flag.
// The float64 centres are the master copy.  A subspace whose flag is set costs every later launch one early return, so
// the host enqueues iterations without reading anything back and looks at the flags every few iterations.
// No float atomics anywhere: labels, centres, iteration counts and scores are the same from run to run and for every
// chunking.
//
// After the loop (cluster_final_kernel, float64 from the raw rows and the float64 centres, one wave per row, lane c on
// centre c): the exactly nearest centre by (d2, index), its d2 (inertia: slice partials, then one ordered sum), the label
// histogram (LDS integer atomics, one global integer add per bin and workgroup) and, once the host has split the
// clusters into large and small ones, the CBLOF score.
#include <limits.h>

#include "outlier_dist.hpp"

namespace vgan {

constexpr int kCMax = VGAN_CLUSTER_MAX_CLUSTERS;
constexpr int kCSlice = VGAN_CLUSTER_SLICE_ROWS;  // rows per slice of the centre sums
constexpr int kCAcc = 4096;                       // float64 accumulators in LDS (32 KiB): threads x C
constexpr int kCFinalRows = 64;                   // rows per workgroup of the final kernel, 16 per wave

// threads of a partial workgroup: every thread needs C private accumulators
static __host__ __device__ inline int cluster_partial_threads(int C) { return C <= 16 ? 256 : (C <= 32 ? 128 : 64); }
static inline int cluster_slices(int n) { return (n + kCSlice - 1) / kCSlice; }

// E step.  Grid (row blocks of 64, 1, chunk subspaces).  label [count, n]; changed[s] += labels that differ from before.
template <bool GRAM>
__global__ __launch_bounds__(kBlock, 2) void cluster_assign_kernel(const float* __restrict__ Pq, const float* __restrict__ sqq, int n,
                                                                   const float* __restrict__ img, const float* __restrict__ img_sq,
                                                                   int C, const int32_t* __restrict__ feat_off,
                                                                   const int64_t* __restrict__ col_off, int first,
                                                                   const int32_t* __restrict__ done, int32_t* __restrict__ label,
                                                                   int32_t* __restrict__ changed) {
    static_assert(DistLds<GRAM>::kFloats >= 2 * kBlock, "merge scratch");
    __shared__ __attribute__((aligned(16))) float lds[DistLds<GRAM>::kFloats];
    const int z = blockIdx.z, s = first + z;
    if (done[s]) return;  // the whole workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x * kOTile + lane;
    float bd = INFINITY;
    int bi = INT_MAX;
    outlier_distances<GRAM>(Pq, sqq, n, img, img_sq, C, feat_off, col_off, first, 1, lds, [&](const float (&d2)[16], int c0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j;
            if (c < C && cand_less(d2[j], c, bd, bi)) {
                bd = d2[j];
                bi = c;
            }
        }
    });
    __syncthreads();
    int* li = reinterpret_cast<int*>(lds) + kBlock;
    lds[tid] = bd;
    li[tid] = bi;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) {
        const float e = lds[w * kWave + lane];
        const int j = li[w * kWave + lane];
        if (cand_less(e, j, bd, bi)) {
            bd = e;
            bi = j;
        }
    }
    if (bi == INT_MAX) bi = 0;  // every distance NaN: any valid label
    int ch = 0;
    if (q < n) {
        const long o = (long)z * n + q;
        ch = label[o] != bi ? 1 : 0;
        label[o] = bi;
    }
    ch = wave_sum(ch);
    if (lane == 0 && ch) atomicAdd(changed + s, ch);
}

// M step, first half.  Grid (slices, feature blocks, chunk subspaces), cluster_partial_threads(C) threads.
// part: subspace z at nb * C * (feat_off[s] - feat_off[first] + z), there [slice][cluster][d_s + 1].
__global__ void cluster_update_partial_kernel(const float* __restrict__ X, int ldx, int n, const int32_t* __restrict__ feat,
                                              const int32_t* __restrict__ feat_off, int first, int C,
                                              const int32_t* __restrict__ label, const int32_t* __restrict__ done,
                                              const int32_t* __restrict__ changed, double* __restrict__ part) {
    __shared__ double acc[kCAcc];
    const int z = blockIdx.z, s = first + z;
    if (done[s] || changed[s] == 0) return;
    const int NT = blockDim.x, tid = threadIdx.x, nb = gridDim.x;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0, wd = ds + 1;
    const int wb = min(wd, NT);  // columns of a feature block; G row groups share the block's threads
    const int fb = blockIdx.y * NT;
    if (fb >= wd) return;
    const int G = NT / wb, g = tid / wb, f = fb + tid % wb;
    const int r0 = blockIdx.x * kCSlice, r1 = min(n, r0 + kCSlice);
    const int32_t* lab = label + (long)z * n;
    for (int c = 0; c < C; ++c) acc[c * NT + tid] = 0.0;
    if (g < G && f < wd) {
        const int col = f < ds ? feat[f0 + f] : -1;
        for (int r = r0 + g; r < r1; r += G) {
            const int l = lab[r];
            const double x = col >= 0 ? (double)X[(long)r * ldx + col] : 1.0;
            if ((unsigned)l < (unsigned)C) acc[l * NT + tid] += x;
        }
    }
    __syncthreads();
    const int nf = min(wb, wd - fb);
    double* out = part + (long)nb * C * (f0 - feat_off[first] + z) + (long)blockIdx.x * C * wd;
    for (int p = tid; p < C * nf; p += NT) {
        const int c = p / nf, ff = p % nf;
        double a = 0.0;
        for (int gg = 0; gg < G; ++gg) a += acc[c * NT + gg * wb + ff];
        out[c * wd + fb + ff] = a;
    }
}

// float32 operand image [C, w_s] of the float64 centres of one subspace (minus the column centre the packed rows were
// centred on, zero padded) and its squared row norms; all threads of the workgroup
__device__ __forceinline__ void cluster_image(const double* __restrict__ cen, int C, int ds, const int32_t* __restrict__ feat,
                                              const float* __restrict__ col_center, float* __restrict__ im, float* __restrict__ sq) {
    const int w = (ds + 3) & ~3;
    auto value = [&](int c, int f) {
        double x = cen[c * ds + f];
        if (col_center != nullptr) x -= (double)col_center[feat[f]];
        return (float)x;
    };
    for (int p = threadIdx.x; p < C * w; p += blockDim.x) {
        const int c = p / w, f = p % w;
        im[p] = f < ds ? value(c, f) : 0.f;
    }
    if (sq != nullptr && threadIdx.x < C) {
        double a = 0.0;
        for (int f = 0; f < ds; ++f) {
            const double v = value(threadIdx.x, f);
            a = fma(v, v, a);
        }
        sq[threadIdx.x] = (float)a;
    }
}

__global__ __launch_bounds__(kBlock) void cluster_image_kernel(const double* __restrict__ centers, int C,
                                                               const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                               const int64_t* __restrict__ col_off, int first,
                                                               const float* __restrict__ col_center, float* __restrict__ img,
                                                               float* __restrict__ img_sq) {
    const int z = blockIdx.x, s = first + z;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0;
    cluster_image(centers + (long)C * f0, C, ds, feat + f0, col_center, img + C * (col_off[s] - col_off[first]),
                  img_sq ? img_sq + (long)z * C : nullptr);
}

// M step, second half; one workgroup per chunk subspace.  An E step that changed nothing ends the subspace (done = 1)
// with no M step; otherwise the centres move (an empty cluster keeps its centre), n_iter counts the step, and a summed
// squared shift <= tol_var[s] (> 0: tol x mean feature variance) ends it (done = 2).
__global__ __launch_bounds__(kBlock) void cluster_update_final_kernel(const double* __restrict__ part, int nb,
                                                                      const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                                      const int64_t* __restrict__ col_off, int first, int C,
                                                                      const float* __restrict__ col_center,
                                                                      const double* __restrict__ tol_var, double* __restrict__ centers,
                                                                      float* __restrict__ img, float* __restrict__ img_sq,
                                                                      int32_t* __restrict__ done, int32_t* __restrict__ changed,
                                                                      int32_t* __restrict__ n_iter) {
    __shared__ double red[4];
    __shared__ double cnt[kCMax];
    const int z = blockIdx.x, s = first + z, tid = threadIdx.x;
    if (done[s]) return;
    const int ch = changed[s];
    __syncthreads();  // every thread has read the count before thread 0 clears it
    if (ch == 0) {
        if (tid == 0) done[s] = 1;
        return;
    }
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0, wd = ds + 1;
    const double* P = part + (long)nb * C * (f0 - feat_off[first] + z);
    if (tid < C) {
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += P[((long)b * C + tid) * wd + ds];
        cnt[tid] = a;
    }
    __syncthreads();
    double* cen = centers + (long)C * f0;
    double shift = 0.0;
    for (int p = tid; p < C * ds; p += kBlock) {
        const int c = p / ds, f = p % ds;
        if (cnt[c] > 0.0) {
            double a = 0.0;
            for (int b = 0; b < nb; ++b) a += P[((long)b * C + c) * wd + f];
            const double nc = a / cnt[c], e = nc - cen[p];
            shift = fma(e, e, shift);
            cen[p] = nc;
        }
    }
    shift = block_sum(shift, red);  // its barrier also orders the centre stores before the image reads them
    cluster_image(cen, C, ds, feat + f0, col_center, img + C * (col_off[s] - col_off[first]), img_sq ? img_sq + (long)z * C : nullptr);
    if (tid == 0) {
        n_iter[s] += 1;
        changed[s] = 0;
        if (tol_var[s] > 0.0 && shift <= tol_var[s]) done[s] = 2;
    }
}

// Float64 assignment and score.  Grid (row blocks of 64, S); wave w takes rows 16 w .. 16 w + 15 of the block, lane c
// centre c.  large == NULL: labels, the block's sum of d2 to the own centre (inertia_part [S, row blocks]) and the label
// histogram (sizes [S, C] += , zeroed by the caller).  large != NULL: labels (label may be NULL) and
// score[score_row[s], q] = sqrt(d2 to the own centre if it is large, else to the nearest large centre) (x sizes[s, label]).
__global__ __launch_bounds__(kBlock) void cluster_final_kernel(const float* __restrict__ Xq, int ldq, int nq,
                                                               const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                               int C, const double* __restrict__ centers,
                                                               const int32_t* __restrict__ large, long long* __restrict__ sizes,
                                                               int use_weights, int32_t* __restrict__ label,
                                                               double* __restrict__ inertia_part, float* __restrict__ score,
                                                               const int32_t* __restrict__ score_row, int ld_score) {
    __shared__ int hist[kCMax];
    __shared__ double wsum[kBlock / kWave];
    const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0;
    const int32_t* F = feat + f0;
    const double* cen = centers + (long)C * f0 + (long)min(lane, C - 1) * ds;
    const bool is_large = large != nullptr && lane < C && large[s * C + lane] != 0;
    if (tid < kCMax) hist[tid] = 0;
    __syncthreads();
    double own_sum = 0.0;
    for (int i = 0; i < kCFinalRows / 4; ++i) {
        const int q = blockIdx.x * kCFinalRows + wave * (kCFinalRows / 4) + i;
        if (q >= nq) break;  // the whole wave
        const float* x = Xq + (long)q * ldq;
        double d2 = 0.0;
        for (int f = 0; f < ds; ++f) {
            const double e = (double)x[F[f]] - cen[f];
            d2 = fma(e, e, d2);
        }
        double bd = lane < C ? d2 : INFINITY;
        int bi = lane < C ? lane : INT_MAX;
        double lm = is_large ? d2 : INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double e = __shfl_xor(bd, o, 64);
            const int j = __shfl_xor(bi, o, 64);
            if (e < bd || (e == bd && j < bi)) {
                bd = e;
                bi = j;
            }
            lm = fmin(lm, __shfl_xor(lm, o, 64));
        }
        bd = __shfl(bd, 0, 64);  // lanes can only disagree on NaN input
        bi = min(__shfl(bi, 0, 64), C - 1);
        own_sum += bd;
        if (lane == 0) {
            if (label != nullptr) label[(long)s * nq + q] = bi;
            if (large == nullptr) {
                atomicAdd(&hist[bi], 1);
            } else {
                double v = sqrt(large[s * C + bi] != 0 ? bd : lm);
                if (use_weights) v *= (double)sizes[s * C + bi];
                score[(long)(score_row ? score_row[s] : s) * ld_score + q] = (float)v;
            }
        }
    }
    if (large != nullptr) return;
    if (lane == 0) wsum[wave] = own_sum;
    __syncthreads();
    if (tid == 0) inertia_part[(long)s * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    if (tid < C && hist[tid]) atomicAdd(reinterpret_cast<unsigned long long*>(sizes) + s * C + tid, (unsigned long long)hist[tid]);
}

// out[r] = sum of row r of src [rows, n] (float64), fixed order; one workgroup per row
__global__ __launch_bounds__(kBlock) void cluster_row_sum_kernel(const double* __restrict__ src, int n, double* __restrict__ out) {
    __shared__ double red[4];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) a += src[(long)blockIdx.x * n + i];
    a = block_sum(a, red);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

static int64_t cluster_part_bytes(int n, int C, int count, int total_dims) {
    return (int64_t)cluster_slices(n) * C * ((int64_t)total_dims + count) * (int64_t)sizeof(double);
}

}  // namespace vgan

using namespace vgan;

extern "C" int64_t vgan_cluster_lloyd_ws_bytes(int n, int n_clusters, int count, int total_dims) {
    if (!(n > 0 && n_clusters >= 2 && n_clusters <= kCMax && count > 0 && total_dims >= count)) {
        set_error("%s:%d: bad argument: n > 0 && 2 <= n_clusters <= 64 && count > 0 && total_dims >= count", __FILE__, __LINE__);
        return -1;
    }
    return cluster_part_bytes(n, n_clusters, count, total_dims);
}

extern "C" int vgan_cluster_image(const double* centers, int n_clusters, const int32_t* feat, const int32_t* feat_off,
                                  const int64_t* col_off, int first, int count, const float* col_center, float* img, float* img_sq,
                                  vgan_stream_t stream) {
    VGAN_CHECK_ARG(centers && feat && feat_off && col_off && img && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(n_clusters >= 2 && n_clusters <= kCMax && aligned16(img));
    hipLaunchKernelGGL(cluster_image_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, centers, n_clusters, feat, feat_off,
                       col_off, first, col_center, img, img_sq);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_cluster_lloyd(const float* Pq, const float* sq_q, const float* X, int ldx, int n, int d, const int32_t* feat,
                                  const int32_t* feat_off, const int64_t* col_off, int first, int count, int total_dims, int max_dims,
                                  int n_clusters, int engine, const float* col_center, const double* tol_var, double* centers,
                                  float* img, float* img_sq, int32_t* label, int32_t* changed, int32_t* done, int32_t* n_iter,
                                  void* workspace, int64_t workspace_bytes, int iterations, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Pq && X && feat && feat_off && col_off && tol_var && centers && img && label && changed && done && n_iter);
    VGAN_CHECK_ARG(n > 0 && d > 0 && ldx >= d && first >= 0 && count > 0 && count <= 65535 && iterations >= 1);
    VGAN_CHECK_ARG(n_clusters >= 2 && n_clusters <= kCMax && n >= n_clusters);
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= d && total_dims >= count && total_dims >= max_dims);
    VGAN_CHECK_ARG(dist_args_ok(engine, sq_q && img_sq, 1, Pq, img) && workspace && aligned16(workspace));
    VGAN_CHECK_ARG(workspace_bytes >= cluster_part_bytes(n, n_clusters, count, total_dims));
    const hipStream_t st = (hipStream_t)stream;
    const int C = n_clusters, nb = cluster_slices(n), nt = cluster_partial_threads(C);
    double* part = static_cast<double*>(workspace);
    const dim3 pgrid(nb, (max_dims + 1 + nt - 1) / nt, count);
    for (int it = 0; it < iterations; ++it) {
        dispatch_engine(engine, [&](auto gram) {
            hipLaunchKernelGGL(cluster_assign_kernel<decltype(gram)::value>, dist_grid(n, 1, count), dim3(kBlock), 0, st, Pq, sq_q, n, img,
                               img_sq, C, feat_off, col_off, first, done, label, changed);
        });
        VGAN_CHECK_LAUNCH();
        hipLaunchKernelGGL(cluster_update_partial_kernel, pgrid, dim3(nt), 0, st, X, ldx, n, feat, feat_off, first, C, label, done,
                           changed, part);
        VGAN_CHECK_LAUNCH();
        hipLaunchKernelGGL(cluster_update_final_kernel, dim3(count), dim3(kBlock), 0, st, part, nb, feat, feat_off, col_off, first, C,
                           col_center, tol_var, centers, img, img_sq, done, changed, n_iter);
        VGAN_CHECK_LAUNCH();
    }
    return VGAN_OK;
}

extern "C" int vgan_cluster_final(const float* Xq, int ldq, int nq, int d, const int32_t* feat, const int32_t* feat_off, int S,
                                  int n_clusters, const double* centers, const int32_t* large, int64_t* sizes, int use_weights,
                                  int32_t* label, double* inertia_part, double* inertia, float* score, const int32_t* score_row,
                                  int ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && feat && feat_off && centers && nq > 0 && d > 0 && ldq >= d && S > 0 && S <= 65535);
    VGAN_CHECK_ARG(n_clusters >= 2 && n_clusters <= kCMax);
    VGAN_CHECK_ARG(large ? (score != nullptr && ld_score >= nq && (!use_weights || sizes)) : (label && sizes && inertia_part && inertia));
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = (nq + kCFinalRows - 1) / kCFinalRows;
    hipLaunchKernelGGL(cluster_final_kernel, dim3(blocks, S), dim3(kBlock), 0, st, Xq, ldq, nq, feat, feat_off, n_clusters, centers,
                       large, reinterpret_cast<long long*>(sizes), use_weights, label, inertia_part, score, score_row, ld_score);
    VGAN_CHECK_LAUNCH();
    if (large == nullptr) {
        hipLaunchKernelGGL(cluster_row_sum_kernel, dim3(S), dim3(kBlock), 0, st, inertia_part, blocks, inertia);
        VGAN_CHECK_LAUNCH();
    }
    return VGAN_OK;
}

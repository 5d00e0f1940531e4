// ECOD (Li, Zhao, Hu, Botta, Ionescu, Chen 2022; pyod's ECOD) over the subspaces: empirical-CDF tail probabilities per
// feature, summed over the features of a subspace.  Nothing here is n x n: fit is one sort per feature, scoring a binary
// search per (row, feature) and one masked sum per (row, subspace).  The per-feature terms do not depend on the subspace,
// so they are formed once and every subspace is a 0/1-masked sum of them: one dense float64 product with the mask [d, S].
//
//   sort     all d columns of X [n, d] at once into sorted [d, n_pad] (n_pad the power of two >= n), a bitonic network on
//            orderable uint32 keys (-0.0 taken as +0.0; the pad key is above every float's).  A run of kEcodRun keys lives
//            in LDS: the head launch sorts every run (all stages up to the run), then per merge size one launch for each
//            stride >= kEcodRun and one tail launch for all strides below it.  The keys stay in the output buffer between
//            launches; the last tail launch decodes them (the pad becomes +inf).  The network is data independent: the
//            result is the unique ascending column, and NaN input cannot change a trip count.
//   skew     one workgroup per column of the sorted image: float64 mean, then m2 and m3 about it, lane-strided partial
//            sums and a fixed butterfly.  sign = 0 if m2 == 0, else the sign of m3.
//   counts   a workgroup takes a 64 x 64 tile of query values through LDS (coalesced in, coalesced out); a wave walks 16
//            columns of it, its 64 lanes searching ONE sorted column for 64 rows, so the probes of a wave share cache lines
//            near the top of the search.  lower and upper bound run in one loop of a fixed number of halvings.
//   terms    counts -> -log(c / n) in float64 (IEEE division, then log), the skew rule, [M rows, d] (M = 1: the
//            elementwise max for "dimension"; M = 3: ul, ur, usk stacked for "tail").
//   product  out^T [S, rows] = mask^T [S, d] x terms^T [d, rows] on v_mfma_f64_16x16x4_f64: ecod_product_kernel of
//            outlier_product.hpp, which the histogram scores (outlier_hist.hip) share.
#include "outlier_product.hpp"

namespace vgan {

constexpr int kEcodRun = VGAN_ECOD_SORT_RUN;  // keys of one LDS-resident run
constexpr int kEcodPairs = 4;                 // compare-exchanges per thread of a strided stage
constexpr int kEcodTile = 64;                 // counts: rows and columns of a staged tile

__device__ __forceinline__ uint32_t ecod_key(float v) {
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ecod_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// position of compare-exchange t of a stage with stride j (a power of two): the lower index of the pair
__device__ __forceinline__ long ecod_pair(long t, long j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// k_merge == 0 (head): keys from X, every stage of the merge sizes 2 .. run.  Otherwise (tail): keys from buf, the stages
// with stride run / 2 .. 1 of merge size k_merge.  decode: the launch is the network's last, buf receives the floats.
__global__ __launch_bounds__(kBlock) void ecod_sort_local_kernel(const float* __restrict__ X, long ldx, int n, uint32_t* __restrict__ buf,
                                                                 long n_pad, int run, long k_merge, int decode) {
    __shared__ uint32_t key[kEcodRun];
    const long col = blockIdx.x, base = (long)blockIdx.y * run;
    uint32_t* out = buf + col * n_pad + base;
    for (int t = threadIdx.x; t < run; t += kBlock) {
        const long i = base + t;
        key[t] = k_merge == 0 ? (i < n ? ecod_key(X[i * ldx + col]) : 0xFFFFFFFFu) : out[t];
    }
    __syncthreads();
    const long k_first = k_merge == 0 ? 2 : k_merge, k_last = k_merge == 0 ? run : k_merge;
    for (long k = k_first; k <= k_last; k <<= 1) {
        for (int j = (int)min(k >> 1, (long)(run >> 1)); j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (run >> 1); t += kBlock) {
                const int i = (int)ecod_pair(t, j);
                const bool ascending = ((base + i) & k) == 0;
                const uint32_t a = key[i], b = key[i + j];
                if ((a > b) == ascending) {
                    key[i] = b;
                    key[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < run; t += kBlock)
        out[t] = decode ? __float_as_uint(base + t < n ? ecod_value(key[t]) : INFINITY) : key[t];
}

// one stage with stride j >= kEcodRun of merge size k; n_pad / 2 pairs a column, kEcodPairs a thread
__global__ __launch_bounds__(kBlock) void ecod_sort_global_kernel(uint32_t* __restrict__ buf, long n_pad, long k, long j) {
    uint32_t* col = buf + (long)blockIdx.x * n_pad;
#pragma unroll
    for (int e = 0; e < kEcodPairs; ++e) {
        const long t = ((long)blockIdx.y * kEcodPairs + e) * kBlock + threadIdx.x;
        const long i = ecod_pair(t, j);
        const bool ascending = (i & k) == 0;
        const uint32_t a = col[i], b = col[i + j];
        if ((a > b) == ascending) {
            col[i] = b;
            col[i + j] = a;
        }
    }
}

__global__ __launch_bounds__(kBlock) void ecod_skew_kernel(const float* __restrict__ sorted, long ld, int n, int8_t* __restrict__ sign) {
    __shared__ double red[kBlock / kWave];
    const float* col = sorted + (long)blockIdx.x * ld;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += (double)col[i];
    const double mu = block_sum_all(s, red) / (double)n;
    double m2 = 0.0, m3 = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const double e = (double)col[i] - mu, e2 = e * e;
        m2 += e2;
        m3 += e2 * e;
    }
    m2 = block_sum_all(m2, red);
    m3 = block_sum_all(m3, red);
    if (threadIdx.x == 0) sign[blockIdx.x] = m2 == 0.0 ? 0 : (int8_t)((m3 > 0.0) - (m3 < 0.0));
}

// cl = #{sorted <= x}, cr = #{sorted >= x} among the first n entries of the column; top: the largest power of two <= n
__global__ __launch_bounds__(kBlock) void ecod_counts_kernel(const float* __restrict__ Xq, long ldq, int rows, int d,
                                                             const float* __restrict__ sorted, long ld, int n, int top,
                                                             int32_t* __restrict__ cl, int32_t* __restrict__ cr) {
    __shared__ float xs[kEcodTile][kEcodTile + 1];
    __shared__ int32_t ls[kEcodTile][kEcodTile + 1], rs[kEcodTile][kEcodTile + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * kEcodTile, c0 = blockIdx.y * kEcodTile;
    for (int row = wave; row < kEcodTile; row += kBlock / kWave)
        xs[row][lane] = (r0 + row < rows && c0 + lane < d) ? Xq[(long)(r0 + row) * ldq + c0 + lane] : 0.f;
    __syncthreads();
    constexpr int per_wave = kEcodTile / (kBlock / kWave);
    for (int cc = 0; cc < per_wave; ++cc) {
        const int ct = wave * per_wave + cc;
        if (c0 + ct >= d) break;  // the same for the whole wave
        float x = xs[lane][ct];
        x = x == 0.f ? 0.f : x;
        const float* col = sorted + (long)(c0 + ct) * ld;
        int below = 0, upto = 0;  // #{< x}, #{<= x}
        for (int step = top; step > 0; step >>= 1) {
            const int p = below + step, q = upto + step;
            const float vp = col[min(p, n) - 1], vq = col[min(q, n) - 1];
            if (p <= n && vp < x) below = p;
            if (q <= n && vq <= x) upto = q;
        }
        ls[lane][ct] = upto;
        rs[lane][ct] = n - below;
    }
    __syncthreads();
    for (int row = wave; row < kEcodTile; row += kBlock / kWave)
        if (r0 + row < rows && c0 + lane < d) {
            const long o = (long)(r0 + row) * d + c0 + lane;
            cl[o] = ls[row][lane];
            cr[o] = rs[row][lane];
        }
}

// counts [rows, d] -> terms [M rows, d]; add = 0 at fit (the row counts itself), 1 for a new row (appended to the n)
template <int M>
__global__ __launch_bounds__(kBlock) void ecod_terms_kernel(const int32_t* __restrict__ cl, const int32_t* __restrict__ cr, long count, int d,
                                                            const int8_t* __restrict__ sign, int n, int add, double* __restrict__ T) {
    const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= count) return;
    const double den = (double)(n + add);
    const double ul = -log((double)(cl[idx] + add) / den), ur = -log((double)(cr[idx] + add) / den);
    const int g = sign[idx % d];
    const double usk = g < 0 ? ul : g > 0 ? ur : ul + ur;
    if (M == 1) {
        T[idx] = fmax(fmax(ul, ur), usk);
    } else {
        T[idx] = ul;
        T[count + idx] = ur;
        T[2 * count + idx] = usk;
    }
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_ecod_sort_columns(const float* X, int ldx, int n, int d, float* sorted, int64_t n_pad, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && sorted && d > 0 && ldx >= d && n >= 1 && n <= VGAN_ECOD_MAX_ROWS);
    VGAN_CHECK_ARG(n_pad >= n && (n_pad & (n_pad - 1)) == 0 && n_pad < 2 * (int64_t)n);
    const hipStream_t st = (hipStream_t)stream;
    uint32_t* buf = reinterpret_cast<uint32_t*>(sorted);
    const int run = (int)(n_pad < kEcodRun ? n_pad : kEcodRun);
    const dim3 local(d, (unsigned)(n_pad / run));
    hipLaunchKernelGGL(ecod_sort_local_kernel, local, dim3(kBlock), 0, st, X, (long)ldx, n, buf, (long)n_pad, run, 0L, n_pad == run ? 1 : 0);
    VGAN_CHECK_LAUNCH();
    for (long k = 2L * run; k <= n_pad; k <<= 1) {
        const dim3 strided(d, (unsigned)(n_pad / 2 / (kEcodPairs * kBlock)));
        for (long j = k >> 1; j >= run; j >>= 1)
            hipLaunchKernelGGL(ecod_sort_global_kernel, strided, dim3(kBlock), 0, st, buf, (long)n_pad, k, j);
        hipLaunchKernelGGL(ecod_sort_local_kernel, local, dim3(kBlock), 0, st, X, (long)ldx, n, buf, (long)n_pad, run, k, k == n_pad ? 1 : 0);
        VGAN_CHECK_LAUNCH();
    }
    return VGAN_OK;
}

extern "C" int vgan_ecod_skew_sign(const float* sorted, int64_t ld, int n, int d, int8_t* sign, vgan_stream_t stream) {
    VGAN_CHECK_ARG(sorted && sign && d > 0 && n >= 1 && n <= VGAN_ECOD_MAX_ROWS && ld >= n);
    hipLaunchKernelGGL(ecod_skew_kernel, dim3(d), dim3(kBlock), 0, (hipStream_t)stream, sorted, (long)ld, n, sign);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ecod_tail_counts(const float* Xq, int ldq, int rows, int d, const float* sorted, int64_t ld, int n, int32_t* cl,
                                     int32_t* cr, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && sorted && cl && cr && rows > 0 && d > 0 && ldq >= d);
    VGAN_CHECK_ARG(n >= 1 && n <= VGAN_ECOD_MAX_ROWS && ld >= n && (d + kEcodTile - 1) / kEcodTile <= 65535);
    int top = 1;
    while (2L * top <= n) top *= 2;
    const dim3 grid((rows + kEcodTile - 1) / kEcodTile, (d + kEcodTile - 1) / kEcodTile);
    hipLaunchKernelGGL(ecod_counts_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, Xq, (long)ldq, rows, d, sorted, (long)ld, n, top, cl, cr);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ecod_scores(const int32_t* cl, const int32_t* cr, int rows, int d, const int8_t* sign, int n, int query,
                                int aggregate, const double* mask, int ldm, int S, double* terms, float* score, int64_t ld_score,
                                vgan_stream_t stream) {
    VGAN_CHECK_ARG(cl && cr && sign && mask && terms && score && rows > 0 && d > 0 && n >= 1 && n <= VGAN_ECOD_MAX_ROWS);
    VGAN_CHECK_ARG(aggregate == VGAN_ECOD_AGGREGATE_DIMENSION || aggregate == VGAN_ECOD_AGGREGATE_TAIL);
    VGAN_CHECK_ARG(S > 0 && ldm >= S && (S + kEcodBS - 1) / kEcodBS <= 65535 && ld_score >= rows);
    const hipStream_t st = (hipStream_t)stream;
    const long count = (long)rows * d;
    const dim3 tgrid((unsigned)((count + kBlock - 1) / kBlock));
    const dim3 pgrid((rows + kEcodBR - 1) / kEcodBR, (S + kEcodBS - 1) / kEcodBS);
    const int add = query ? 1 : 0;
    if (aggregate == VGAN_ECOD_AGGREGATE_DIMENSION) {
        hipLaunchKernelGGL(ecod_terms_kernel<1>, tgrid, dim3(kBlock), 0, st, cl, cr, count, d, sign, n, add, terms);
        hipLaunchKernelGGL(ecod_product_kernel<1>, pgrid, dim3(kBlock), 0, st, terms, (long)rows, d, mask, ldm, S, score, (long)ld_score);
    } else {
        hipLaunchKernelGGL(ecod_terms_kernel<3>, tgrid, dim3(kBlock), 0, st, cl, cr, count, d, sign, n, add, terms);
        hipLaunchKernelGGL(ecod_product_kernel<3>, pgrid, dim3(kBlock), 0, st, terms, (long)rows, d, mask, ldm, S, score, (long)ld_score);
    }
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

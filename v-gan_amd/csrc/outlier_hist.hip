// Histogram outlier scores over the subspaces: HBOS (Goldstein and Dengel 2012; pyod's HBOS) and LODA (Pevny 2016; pyod's
// LODA).  Both are linear in n: no n x n sweep, no sort, no factorisation.  One histogram engine serves both: the range of
// a column, its equal-width edges, exact integer counts and the bin of a value.  A "column" is a feature of X (HBOS, P = d
// columns of float32) or the projected value z of one sparse random projection of one subspace (LODA, P = S k columns of
// float64, never stored: z is recomputed by the range, the count and the scoring launch).
//
//   range    min and max of every column as integer atomics on order-preserving 64-bit keys of the float64 value (-0.0
//            taken as +0.0): a min or a max is exact in any order.  keys [P, 2].  HBOS: a workgroup reads rows of X
//            coalesced over a tile of 64 columns, a column a lane, and merges its four waves in LDS before the atomics.
//   edges    one thread per (column, j): lo == hi becomes (lo - 0.5, lo + 0.5); step = (hi - lo) / B; e_j = j * step + lo
//            as TWO roundings (mul_rounded: the library is built with -ffp-contract=fast, which would otherwise fuse
//            them); e_B = hi.  numpy.linspace(lo, hi, B + 1) bit for bit.
//   bin      #{j in 1 .. B - 1 : e_j <= x}: a search of eight fixed halvings (B <= 256) whose every probe is clamped, so
//            that NaN input or NaN edges change no trip count and reach no index outside the table.
//   counts   an LDS integer histogram per workgroup (a tile of columns over a slab of rows), LDS integer atomics, flushed
//            with global integer atomics: integer sums only, exact and free of any order.  There is no float atomic here.
//   HBOS     the term of every (row, feature) is looked up in a table the host built in float64 from the counts (term_f[b],
//            then the out-of-range term; the limits lo - tol step and hi + tol step come from the host too, so no product
//            here is left to contraction): T [rows, d]; then the masked product T x mask [d, S] of outlier_product.hpp.
//   LODA     a workgroup takes one subspace and a slab of rows of its PACKED block (outlier.hip's vgan_outlier_pack: the
//            subspace's features of a row are contiguous), staged through LDS a few rows at a time.  A wave takes a row, its
//            lanes the projections j = lane, lane + 64, ...; the nonzeros of a projection are stored t-major ([m_s, k]), so
//            the 64 lanes read neighbouring entries.  z = (((0 + w_0 x_0) + w_1 x_1) + ...) with every product and every
//            sum rounded on its own (mul_rounded, for the same reason as the edges).  Range and counts gather in
//            LDS (64-bit min / max, integer adds) and flush with global integer atomics; the score of a row is the lanes'
//            partial sums over j ascending, then the wave butterfly: an order fixed by k alone.
#include "outlier_product.hpp"

namespace vgan {

constexpr int kHistMaxBins = VGAN_HIST_MAX_BINS;
constexpr int kHistSlabRows = 1024;  // rows of X one workgroup of the column kernels walks
constexpr int kHistCountCols = 16;   // columns of one counting workgroup: edges and counts of the tile live in LDS
constexpr int kLodaStage = VGAN_LODA_MAX_DIMS;  // floats of the staged rows: at least one row of the widest subspace
constexpr int kLodaTileRows = 16;               // rows staged at a time, at most
constexpr int kLodaSlabRows = 128;              // rows of one workgroup
constexpr int kLodaAcc = 2 * VGAN_LODA_MAX_PROJECTIONS;  // 64-bit words: a (min, max) pair a projection, or 2 kLodaAcc int32 counts

typedef unsigned long long u64;

// order-preserving key of a float64 (NaN sorts above or below every number by its sign)
__device__ __forceinline__ u64 hist_key(double v) {
    const u64 u = (u64)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double hist_value(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// the bin of x among the edges e[0 .. B]: #{j in 1 .. B - 1 : e[j] <= x}; eight steps, every probe inside 1 .. B - 1
__device__ __forceinline__ int hist_bin(const double* e, int B, double x) {
    int pos = 0;
#pragma unroll
    for (int step = kHistMaxBins / 2; step > 0; step >>= 1) {
        const int p = pos + step;
        const double v = e[min(p, B - 1)];
        if (p <= B - 1 && v <= x) pos = p;
    }
    return pos;
}

__global__ __launch_bounds__(kBlock) void hist_keys_init_kernel(u64* __restrict__ keys, long P) {
    const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (idx < 2 * P) keys[idx] = (idx & 1) ? 0ull : ~0ull;  // min above every key, max below
}

__global__ __launch_bounds__(kBlock) void hist_zero_kernel(int32_t* __restrict__ counts, long cells) {
    const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (idx < cells) counts[idx] = 0;
}

__global__ __launch_bounds__(kBlock) void hist_column_range_kernel(const float* __restrict__ X, long ldx, int n, int d, u64* __restrict__ keys) {
    __shared__ u64 lo_s[kBlock / kWave][kWave], hi_s[kBlock / kWave][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * kWave + lane;
    const int r0 = blockIdx.y * kHistSlabRows, r1 = min(n, r0 + kHistSlabRows);
    u64 lo = ~0ull, hi = 0ull;
    if (c < d)
        for (int r = r0 + wave; r < r1; r += kBlock / kWave) {
            const float x = X[(long)r * ldx + c];
            const u64 key = hist_key(x == 0.f ? 0.0 : (double)x);
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
        }
    lo_s[wave][lane] = lo;
    hi_s[wave][lane] = hi;
    __syncthreads();
    if (wave == 0 && c < d) {
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) {
            lo = lo_s[w][lane] < lo ? lo_s[w][lane] : lo;
            hi = hi_s[w][lane] > hi ? hi_s[w][lane] : hi;
        }
        atomicMin(&keys[2L * c], lo);
        atomicMax(&keys[2L * c + 1], hi);
    }
}

__global__ __launch_bounds__(kBlock) void hist_edges_kernel(const u64* __restrict__ keys, long P, int B, double* __restrict__ edges) {
    const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= P * (B + 1)) return;
    const long p = idx / (B + 1);
    const int j = (int)(idx % (B + 1));
    double lo = hist_value(keys[2 * p]), hi = hist_value(keys[2 * p + 1]);
    if (lo == hi) {  // numpy.histogram's range of a constant column
        hi = lo + 0.5;
        lo = lo - 0.5;
    }
    const double step = (hi - lo) / (double)B;
    // two roundings, as numpy.linspace takes them: the product, then the sum
    edges[idx] = j == B ? hi : mul_rounded((double)j, step) + lo;
}

__global__ __launch_bounds__(kBlock) void hist_column_counts_kernel(const float* __restrict__ X, long ldx, int n, int d,
                                                                   const double* __restrict__ edges, int B, int32_t* __restrict__ counts) {
    __shared__ double le[kHistCountCols][kHistMaxBins + 1];
    __shared__ int lh[kHistCountCols][kHistMaxBins];
    const int tid = threadIdx.x, ct = tid % kHistCountCols, rt = tid / kHistCountCols;
    const int c0 = blockIdx.x * kHistCountCols, cols = min(kHistCountCols, d - c0);
    const int r0 = blockIdx.y * kHistSlabRows, r1 = min(n, r0 + kHistSlabRows);
    for (int e = tid; e < cols * (B + 1); e += kBlock) le[e / (B + 1)][e % (B + 1)] = edges[(long)c0 * (B + 1) + e];
    for (int e = tid; e < cols * B; e += kBlock) lh[e / B][e % B] = 0;
    __syncthreads();
    if (ct < cols)
        for (int r = r0 + rt; r < r1; r += kBlock / kHistCountCols) {
            const float x = X[(long)r * ldx + c0 + ct];
            atomicAdd(&lh[ct][hist_bin(le[ct], B, x == 0.f ? 0.0 : (double)x)], 1);
        }
    __syncthreads();
    for (int e = tid; e < cols * B; e += kBlock) {
        const int v = lh[e / B][e % B];
        if (v) atomicAdd(&counts[(long)c0 * B + e], v);
    }
}

// T [rows, d]: table [d, B + 1] holds term_f[0 .. B - 1] and then the out-of-range term; limits [d, 2] the two thresholds
__global__ __launch_bounds__(kBlock) void hbos_terms_kernel(const float* __restrict__ Xq, long ldq, long count, int d,
                                                           const double* __restrict__ edges, int B, const double* __restrict__ table,
                                                           const double* __restrict__ limits, double* __restrict__ T) {
    const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= count) return;
    const long r = idx / d;
    const int c = (int)(idx % d);
    const float xf = Xq[r * ldq + c];
    const double x = xf == 0.f ? 0.0 : (double)xf;
    const int bin = hist_bin(edges + (long)c * (B + 1), B, x);
    const bool outside = x < limits[2 * c] || x > limits[2 * c + 1];
    T[idx] = table[(long)c * (B + 1) + (outside ? B : bin)];
}

// MODE 0: keys (min, max) of z; 1: counts of the bins of z; 2: the scores.  grid (row slabs, subspaces, projection tiles of
// kt; only the counts are tiled, by what their LDS histogram holds)
template <int MODE>
__global__ __launch_bounds__(kBlock) void loda_kernel(const float* __restrict__ P, int rows, const int32_t* __restrict__ feat_off,
                                                      const int64_t* __restrict__ col_off, int first, const int32_t* __restrict__ pidx,
                                                      const double* __restrict__ pw, const int64_t* __restrict__ moff, int k, int kt,
                                                      const double* __restrict__ edges, int B, const double* __restrict__ terms,
                                                      u64* __restrict__ keys, int32_t* __restrict__ counts, float* __restrict__ score,
                                                      long ld_score) {
    __shared__ float xs[kLodaStage];
    __shared__ u64 lacc[MODE == 2 ? 1 : kLodaAcc];
    int* lh = reinterpret_cast<int*>(lacc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = first + blockIdx.y;
    const int ds = feat_off[s + 1] - feat_off[s], w = (int)(col_off[s + 1] - col_off[s]), m = (int)(moff[s + 1] - moff[s]);
    if (w < 1 || w > kLodaStage || ds < 1) return;  // the same for the whole workgroup: a row must fit the stage
    const float* Ps = P + (long)rows * (col_off[s] - col_off[first]);
    const int32_t* pi = pidx + (long)k * moff[s];
    const double* pv = pw + (long)k * moff[s];
    const int j0 = blockIdx.z * kt, j1 = min(k, j0 + kt);
    const int tile = min(kLodaTileRows, kLodaStage / w);
    const int r0 = blockIdx.x * kLodaSlabRows, r1 = min(rows, r0 + kLodaSlabRows);
    if (MODE == 0)
        for (int e = tid; e < 2 * (j1 - j0); e += kBlock) lacc[e] = (e & 1) ? 0ull : ~0ull;
    if (MODE == 1)
        for (int e = tid; e < (j1 - j0) * B; e += kBlock) lh[e] = 0;
    for (int t0 = r0; t0 < r1; t0 += tile) {
        const int nt = min(tile, r1 - t0);
        __syncthreads();  // the previous tile has been read (and the accumulators are set)
        for (int e = tid; e < nt * w; e += kBlock) xs[e] = Ps[(long)t0 * w + e];
        __syncthreads();
        for (int r = wave; r < nt; r += kBlock / kWave) {
            const float* x = xs + r * w;
            double total = 0.0;
            for (int j = j0 + lane; j < j1; j += kWave) {
                double z = 0.0;
                for (int t = 0; t < m; ++t) {
                    const int f = min(max(pi[(long)t * k + j], 0), ds - 1);
                    // every product and every sum rounded on its own, as numpy's acc = acc + w * x
                    z = z + mul_rounded(pv[(long)t * k + j], (double)x[f]);
                }
                const long col = (long)s * k + j;
                if (MODE == 0) {
                    const u64 key = hist_key(z);
                    atomicMin(&lacc[2 * (j - j0)], key);
                    atomicMax(&lacc[2 * (j - j0) + 1], key);
                } else {
                    const int bin = hist_bin(edges + col * (B + 1), B, z);
                    if (MODE == 1)
                        atomicAdd(&lh[(j - j0) * B + bin], 1);
                    else
                        total += terms[col * B + bin];
                }
            }
            if (MODE == 2) {
                total = wave_sum(total);
                if (lane == 0) score[(long)s * ld_score + t0 + r] = (float)((1.0 / (double)k) * total);
            }
        }
    }
    __syncthreads();
    if (MODE == 0)
        for (int e = tid; e < j1 - j0; e += kBlock) {
            atomicMin(&keys[2 * ((long)s * k + j0 + e)], lacc[2 * e]);
            atomicMax(&keys[2 * ((long)s * k + j0 + e) + 1], lacc[2 * e + 1]);
        }
    if (MODE == 1)
        for (int e = tid; e < (j1 - j0) * B; e += kBlock)
            if (lh[e]) atomicAdd(&counts[((long)s * k + j0) * B + e], lh[e]);
}

inline unsigned blocks_for(long count) { return (unsigned)((count + kBlock - 1) / kBlock); }

inline bool loda_range_ok(const void* P, int rows, const void* feat_off, const void* col_off, int first, int count, int max_dims,
                          const void* pidx, const void* pw, const void* moff, int k) {
    return P && feat_off && col_off && pidx && pw && moff && rows > 0 && rows <= VGAN_HIST_MAX_ROWS && first >= 0 && count > 0 &&
           count <= 65535 && max_dims >= 1 && max_dims <= VGAN_LODA_MAX_DIMS && k >= 1 && k <= VGAN_LODA_MAX_PROJECTIONS;
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_hist_column_range(const float* X, int ldx, int n, int d, uint64_t* keys, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && keys && d > 0 && ldx >= d && n >= 1 && n <= VGAN_HIST_MAX_ROWS);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hist_keys_init_kernel, dim3(blocks_for(2L * d)), dim3(kBlock), 0, st, (u64*)keys, (long)d);
    const dim3 grid((d + kWave - 1) / kWave, (n + kHistSlabRows - 1) / kHistSlabRows);
    hipLaunchKernelGGL(hist_column_range_kernel, grid, dim3(kBlock), 0, st, X, (long)ldx, n, d, (u64*)keys);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_hist_edges(const uint64_t* keys, int64_t P, int B, double* edges, vgan_stream_t stream) {
    VGAN_CHECK_ARG(keys && edges && P >= 1 && B >= 2 && B <= VGAN_HIST_MAX_BINS && P <= (1LL << 31) / (B + 1));
    hipLaunchKernelGGL(hist_edges_kernel, dim3(blocks_for(P * (B + 1))), dim3(kBlock), 0, (hipStream_t)stream, (const u64*)keys, (long)P, B,
                       edges);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_hist_column_counts(const float* X, int ldx, int n, int d, const double* edges, int B, int32_t* counts,
                                       vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && edges && counts && d > 0 && ldx >= d && n >= 1 && n <= VGAN_HIST_MAX_ROWS && B >= 2 && B <= VGAN_HIST_MAX_BINS);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hist_zero_kernel, dim3(blocks_for((long)d * B)), dim3(kBlock), 0, st, counts, (long)d * B);
    const dim3 grid((d + kHistCountCols - 1) / kHistCountCols, (n + kHistSlabRows - 1) / kHistSlabRows);
    hipLaunchKernelGGL(hist_column_counts_kernel, grid, dim3(kBlock), 0, st, X, (long)ldx, n, d, edges, B, counts);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_hbos_scores(const float* Xq, int ldq, int rows, int d, const double* edges, int B, const double* table,
                                const double* limits, const double* mask, int ldm, int S, double* terms, float* score, int64_t ld_score,
                                vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && edges && table && limits && mask && terms && score && rows > 0 && d > 0 && ldq >= d);
    VGAN_CHECK_ARG(B >= 2 && B <= VGAN_HIST_MAX_BINS && S > 0 && ldm >= S && (S + kEcodBS - 1) / kEcodBS <= 65535 && ld_score >= rows);
    const hipStream_t st = (hipStream_t)stream;
    const long count = (long)rows * d;
    hipLaunchKernelGGL(hbos_terms_kernel, dim3(blocks_for(count)), dim3(kBlock), 0, st, Xq, (long)ldq, count, d, edges, B, table, limits, terms);
    const dim3 pgrid((rows + kEcodBR - 1) / kEcodBR, (S + kEcodBS - 1) / kEcodBS);
    hipLaunchKernelGGL(ecod_product_kernel<1>, pgrid, dim3(kBlock), 0, st, terms, (long)rows, d, mask, ldm, S, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_hist_reset(uint64_t* keys, int64_t P, int32_t* counts, int64_t cells, vgan_stream_t stream) {
    VGAN_CHECK_ARG((keys || counts) && (!keys || P >= 1) && (!counts || cells >= 1));
    const hipStream_t st = (hipStream_t)stream;
    if (keys) hipLaunchKernelGGL(hist_keys_init_kernel, dim3(blocks_for(2 * P)), dim3(kBlock), 0, st, (u64*)keys, (long)P);
    if (counts) hipLaunchKernelGGL(hist_zero_kernel, dim3(blocks_for(cells)), dim3(kBlock), 0, st, counts, (long)cells);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_loda_range(const float* P, int rows, const int32_t* feat_off, const int64_t* col_off, int first, int count,
                               int max_dims, const int32_t* pidx, const double* pw, const int64_t* moff, int k, uint64_t* keys,
                               vgan_stream_t stream) {
    VGAN_CHECK_ARG(loda_range_ok(P, rows, feat_off, col_off, first, count, max_dims, pidx, pw, moff, k) && keys);
    const dim3 grid((rows + kLodaSlabRows - 1) / kLodaSlabRows, count, 1);
    hipLaunchKernelGGL(loda_kernel<0>, grid, dim3(kBlock), 0, (hipStream_t)stream, P, rows, feat_off, col_off, first, pidx, pw, moff, k, k,
                       (const double*)nullptr, 2, (const double*)nullptr, (u64*)keys, (int32_t*)nullptr, (float*)nullptr, 0L);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_loda_counts(const float* P, int rows, const int32_t* feat_off, const int64_t* col_off, int first, int count,
                                int max_dims, const int32_t* pidx, const double* pw, const int64_t* moff, int k, const double* edges,
                                int B, int32_t* counts, vgan_stream_t stream) {
    VGAN_CHECK_ARG(loda_range_ok(P, rows, feat_off, col_off, first, count, max_dims, pidx, pw, moff, k) && edges && counts);
    VGAN_CHECK_ARG(B >= 2 && B <= VGAN_HIST_MAX_BINS);
    const int kt = 2 * kLodaAcc / B;  // projections whose counts fit the LDS histogram: at least 16
    const dim3 grid((rows + kLodaSlabRows - 1) / kLodaSlabRows, count, (k + kt - 1) / kt);
    hipLaunchKernelGGL(loda_kernel<1>, grid, dim3(kBlock), 0, (hipStream_t)stream, P, rows, feat_off, col_off, first, pidx, pw, moff, k, kt,
                       edges, B, (const double*)nullptr, (u64*)nullptr, counts, (float*)nullptr, 0L);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_loda_scores(const float* P, int rows, const int32_t* feat_off, const int64_t* col_off, int first, int count,
                                int max_dims, const int32_t* pidx, const double* pw, const int64_t* moff, int k, const double* edges,
                                int B, const double* terms, float* score, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(loda_range_ok(P, rows, feat_off, col_off, first, count, max_dims, pidx, pw, moff, k) && edges && terms && score);
    VGAN_CHECK_ARG(B >= 2 && B <= VGAN_HIST_MAX_BINS && ld_score >= rows);
    const dim3 grid((rows + kLodaSlabRows - 1) / kLodaSlabRows, count, 1);
    hipLaunchKernelGGL(loda_kernel<2>, grid, dim3(kBlock), 0, (hipStream_t)stream, P, rows, feat_off, col_off, first, pidx, pw, moff, k, k,
                       edges, B, terms, (u64*)nullptr, (int32_t*)nullptr, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

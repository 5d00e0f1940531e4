// RS-Hash (Sathe and Aggarwal, "Subspace Outlier Detection in Linear Time with Randomized Hashing", ICDM 2016) over the
// subspaces: T components per subspace, each a randomly shifted grid of width f over r of the subspace's features, holding
// the counts of s sampled rows per occupied cell; a row's score falls with the log of the count of its own cell.  Nothing
// here is n x n, nothing is a tree or a moment: the build touches s rows per component, scoring is r gathers and one binary
// search per (row, component).  Every number up to the final division is an integer.
//
//   digit    of a value x of chosen feature j: x' = (x - mn_j) / w_j (0 where w_j = mx_j - mn_j is 0), y = floor((x' +
//            alpha_j) / f) clamped to [-1, floor(1 / f) + 2], digit = y + 1; float64 on the float32 values, a subtraction, two
//            divisions and a sum, nothing fused.  R = floor(1 / f) + 4; key = sum_j digit_j R^j as uint64.
//   build    one workgroup per component.  The s sampled row indices (feistel_perm of the component's stream) and then the
//            keys live in LDS (4 + 8 bytes a row of the padded sample, 48 KB at s = 4096); the indices are sorted (bitonic,
//            padded to a power of two) and, when asked for, stored: the fit's in-sample test searches them.  Per chosen
//            feature the float32 min and max over the sample (-0.0 as +0.0) are a workgroup reduction; the keys are formed,
//            sorted by the same network and compacted by a scan over the run heads into distinct keys (ascending, padding
//            2^64 - 1) and counts (padding 0).
//   sums     a workgroup owns one subspace and R x kBlock query rows (R = 1 or 4) and walks the subspace's T components: it
//            stages a component's keys, counts (as 16 bits: a count is at most 4096) and parameters through LDS, at fit
//            also the sorted sample indices (10 or 14 bytes a sampled row, sized by s at the launch: 14 KB at s = 1000).
//            A lane forms the key of its row with r gathers (X through two strides: row-major as given, or a column-major
//            copy), finds it by a branchless lower bound in LDS, at fit looks its own row index up among the sample, and
//            adds table[c] to an int64 register.  A component without features (a subspace whose features are all
//            constant) adds table[s + 1], so that the score below is exactly 0.
//   scores   float32(1 - double(sum) / double(denom)), denom = T table[s + 1].
#include "vgan_common.hpp"

namespace vgan {

typedef unsigned long long u64;

constexpr int kRsMaxSamples = VGAN_RSHASH_MAX_SAMPLES;  // s
constexpr int kRsMaxDims = VGAN_RSHASH_MAX_DIMS;        // r
constexpr int kRsWaves = kBlock / kWave;
constexpr u64 kRsPadKey = ~0ull;

__device__ __forceinline__ float rs_value(float v) { return v == 0.f ? 0.f : v; }  // -0.0 as +0.0

// R and the upper clamp of y from the grid width; f lies in [1 / 64, 63 / 64], anything else is held to that range's radices
__device__ __forceinline__ int rs_radix(double f) {
    const double q = floor(1.0 / f);
    return (q >= 1.0 && q <= 64.0 ? (int)q : 1) + 4;
}

__device__ __forceinline__ u64 rs_digit(float x, double mn, double w, double shift, double f, double top) {
    double t = 0.0;
    if (w > 0.0) t = ((double)x - mn) / w;
    double y = floor((t + shift) / f);
    y = fmin(fmax(y, -1.0), top);  // NaN goes to -1
    return (u64)((long long)y + 1);
}

// the power of two the sort of s elements is padded to
__host__ __device__ inline int rs_padded(int s) {
    int P = 2;
    while (P < s) P <<= 1;
    return P;
}

// ascending bitonic network over a[0 .. P), P a power of two, by the whole workgroup; ends with a barrier
template <typename K>
__device__ __forceinline__ void rs_bitonic(K* a, int P) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += kBlock) {
                const int l = i ^ j;
                if (l > i) {
                    const K x = a[i], y = a[l];
                    if ((x > y) == ((i & k) == 0)) {
                        a[i] = y;
                        a[l] = x;
                    }
                }
            }
            __syncthreads();
        }
}

struct RsComponents {
    const int32_t* dims;    // [S, T]
    const int32_t* feat;    // [S, T, kRsMaxDims] columns of X
    const double* shift;    // [S, T, kRsMaxDims]
    const double* width;    // [S, T]
};

struct RsState {
    u64* key;          // [S, T, s]
    int32_t* count;    // [S, T, s]
    int32_t* n_cells;  // [S, T]
    float* mn;         // [S, T, kRsMaxDims]
    float* mx;         // [S, T, kRsMaxDims]
    int32_t* sample;   // [S, T, s] or NULL
};

__global__ __launch_bounds__(kBlock) void rshash_build_kernel(const float* __restrict__ X, long ldx, u64 n, int d, int first, int T, int s,
                                                              int w, u64 seed, RsComponents comp, RsState st) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_build_lds[];  // P keys, then P row indices
    __shared__ float red_lo[kRsMaxDims][kRsWaves], red_hi[kRsMaxDims][kRsWaves];
    __shared__ double p_mn[kRsMaxDims], p_w[kRsMaxDims], p_shift[kRsMaxDims];
    __shared__ int p_col[kRsMaxDims];
    __shared__ int scan[kBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long c = (long)(first + (int)(blockIdx.x / (unsigned)T)) * T + (long)(blockIdx.x % (unsigned)T);
    const int r = min(max(comp.dims[c], 0), kRsMaxDims);
    const int P = rs_padded(s);
    u64* keys = reinterpret_cast<u64*>(rs_build_lds);
    int* rows = reinterpret_cast<int*>(keys + P);

    for (int i = tid; i < P; i += kBlock) rows[i] = i < s ? (int)feistel_perm((u64)i, n, w, seed, (u64)c) : 0x7FFFFFFF;
    __syncthreads();
    rs_bitonic(rows, P);
    if (st.sample)
        for (int i = tid; i < s; i += kBlock) st.sample[c * s + i] = rows[i];
    if (tid < kRsMaxDims) {
        p_col[tid] = tid < r ? min(max(comp.feat[c * kRsMaxDims + tid], 0), d - 1) : 0;
        p_shift[tid] = tid < r ? comp.shift[c * kRsMaxDims + tid] : 0.0;
    }
    __syncthreads();

    for (int j = 0; j < r; ++j) {
        const long col = p_col[j];
        float lo = INFINITY, hi = -INFINITY;
        for (int i = tid; i < s; i += kBlock) {
            const float x = rs_value(X[(long)rows[i] * ldx + col]);
            lo = fminf(lo, x);
            hi = fmaxf(hi, x);
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        if (lane == 0) {
            red_lo[j][wave] = lo;
            red_hi[j][wave] = hi;
        }
    }
    __syncthreads();
    if (tid < kRsMaxDims) {
        float lo = 0.f, hi = 0.f;
        if (tid < r) {
            lo = fminf(fminf(red_lo[tid][0], red_lo[tid][1]), fminf(red_lo[tid][2], red_lo[tid][3]));
            hi = fmaxf(fmaxf(red_hi[tid][0], red_hi[tid][1]), fmaxf(red_hi[tid][2], red_hi[tid][3]));
        }
        p_mn[tid] = (double)lo;
        p_w[tid] = (double)hi - (double)lo;
        st.mn[c * kRsMaxDims + tid] = lo;
        st.mx[c * kRsMaxDims + tid] = hi;
    }
    __syncthreads();

    const double f = comp.width[c];
    const int radix = rs_radix(f);
    const double top = (double)(radix - 2);
    for (int i = tid; i < P; i += kBlock) {
        u64 key = kRsPadKey;
        if (i < s) {
            key = 0;
            u64 mult = 1;
            for (int j = 0; j < r; ++j) {
                key += rs_digit(X[(long)rows[i] * ldx + p_col[j]], p_mn[j], p_w[j], p_shift[j], f, top) * mult;
                mult *= (u64)radix;
            }
        }
        keys[i] = key;
    }
    __syncthreads();
    rs_bitonic(keys, P);

    // run heads of keys[0 .. s): a contiguous slice a thread, an exclusive scan of the slices' head counts
    const int per = (s + kBlock - 1) / kBlock;
    const int i0 = min(tid * per, s), i1 = min(i0 + per, s);
    int heads = 0;
    for (int i = i0; i < i1; ++i) heads += (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
    scan[tid] = heads;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const int v = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const int cells = r > 0 ? scan[kBlock - 1] : 0;
    int pos = scan[tid] - heads;
    int* starts = rows;  // the sample indices are not needed any more
    if (r > 0)
        for (int i = i0; i < i1; ++i)
            if (i == 0 || keys[i] != keys[i - 1]) {
                starts[pos] = i;
                st.key[c * s + pos] = keys[i];
                ++pos;
            }
    __syncthreads();
    for (int p = tid; p < s; p += kBlock) {
        if (p < cells) {
            st.count[c * s + p] = (p + 1 < cells ? starts[p + 1] : s) - starts[p];
        } else {
            st.key[c * s + p] = kRsPadKey;
            st.count[c * s + p] = 0;
        }
    }
    if (tid == 0) st.n_cells[c] = cells;
}

struct RsFitted {
    const u64* key;
    const int32_t* count;
    const int32_t* n_cells;
    const float* mn;
    const float* mx;
    const int32_t* sample;  // NULL: new rows, every count gets plus 1
};

template <int R, bool FIT>
__global__ __launch_bounds__(kBlock) void rshash_sums_kernel(const float* __restrict__ Xq, long row_stride, long col_stride, int nrows, int d,
                                                             long row_base, int first, int T, int s, RsComponents comp, RsFitted st,
                                                             const int64_t* __restrict__ table, int64_t* __restrict__ sums, long ld_sums) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_sums_lds[];  // sp keys, FIT: sp sample rows, sp counts
    const int sp = (s + 3) & ~3;
    u64* keys = reinterpret_cast<u64*>(rs_sums_lds);
    int* samp = reinterpret_cast<int*>(keys + sp);
    unsigned short* cnts = reinterpret_cast<unsigned short*>(samp + (FIT ? sp : 0));
    __shared__ double p_mn[kRsMaxDims], p_w[kRsMaxDims], p_shift[kRsMaxDims];
    __shared__ long p_col[kRsMaxDims];
    const int tid = threadIdx.x;
    const int z = blockIdx.y;
    long at[R], self[R];
    int64_t total[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const long row = min((long)blockIdx.x * (R * kBlock) + tid + (long)q * kBlock, (long)nrows - 1);  // a surplus lane repeats the last row
        at[q] = row * row_stride;
        self[q] = row_base + row;
        total[q] = 0;
    }
    const int64_t empty = table[s + 1];
    int sstep = 1;  // the largest power of two <= s
    while (2 * sstep <= s) sstep <<= 1;
    for (int t = 0; t < T; ++t) {
        const long c = (long)(first + z) * T + t;
        const int r = min(max(comp.dims[c], 0), kRsMaxDims);
        if (r == 0) {  // the same for the whole workgroup
#pragma unroll
            for (int q = 0; q < R; ++q) total[q] += empty;
            continue;
        }
        const int cells = min(max(st.n_cells[c], 0), s);
        __syncthreads();  // the previous component has been searched
        for (int i = tid; i < cells; i += kBlock) {
            keys[i] = st.key[c * s + i];
            cnts[i] = (unsigned short)min(max(st.count[c * s + i], 0), s);
        }
        if (FIT)
            for (int i = tid; i < s; i += kBlock) samp[i] = st.sample[c * s + i];
        if (tid < r) {
            const double lo = (double)st.mn[c * kRsMaxDims + tid], hi = (double)st.mx[c * kRsMaxDims + tid];
            p_mn[tid] = lo;
            p_w[tid] = hi - lo;
            p_shift[tid] = comp.shift[c * kRsMaxDims + tid];
            p_col[tid] = (long)min(max(comp.feat[c * kRsMaxDims + tid], 0), d - 1) * col_stride;
        }
        __syncthreads();
        const double f = comp.width[c];
        const int radix = rs_radix(f);
        const double top = (double)(radix - 2);
        int cstep = 1;
        while (2 * cstep <= cells) cstep <<= 1;
        u64 key[R];
#pragma unroll
        for (int q = 0; q < R; ++q) key[q] = 0;
        u64 mult = 1;
        for (int j = 0; j < r; ++j) {
            float x[R];
#pragma unroll
            for (int q = 0; q < R; ++q) x[q] = Xq[at[q] + p_col[j]];
#pragma unroll
            for (int q = 0; q < R; ++q) key[q] += rs_digit(x[q], p_mn[j], p_w[j], p_shift[j], f, top) * mult;
            mult *= (u64)radix;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            int pos = 0;  // the number of keys below key[q]
            for (int step = cstep; step > 0; step >>= 1) {
                const int e = pos + step;
                if (e <= cells && keys[e - 1] < key[q]) pos = e;
            }
            int cnt = (pos < cells && keys[pos] == key[q]) ? (int)cnts[pos] : 0;
            if (FIT) {
                int sp = 0;
                for (int step = sstep; step > 0; step >>= 1) {
                    const int e = sp + step;
                    if (e <= s && (long)samp[e - 1] < self[q]) sp = e;
                }
                cnt += (sp < s && (long)samp[sp] == self[q]) ? 0 : 1;
            } else {
                cnt += 1;
            }
            total[q] += table[min(cnt, s + 1)];
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const long row = (long)blockIdx.x * (R * kBlock) + tid + (long)q * kBlock;
        if (row < nrows) sums[(long)z * ld_sums + row] = total[q];
    }
}

__global__ __launch_bounds__(kBlock) void rshash_scores_kernel(const int64_t* __restrict__ sums, long ld_sums, int rows, double denom,
                                                               float* __restrict__ score, long ld_score) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    const long z = blockIdx.y;
    if (i < rows) score[z * ld_score + i] = (float)(1.0 - (double)sums[z * ld_sums + i] / denom);
}

}  // namespace vgan

using namespace vgan;

static bool rshash_shape_ok(int T, int s) { return T >= 1 && T <= VGAN_RSHASH_MAX_COMPONENTS && s >= 2 && s <= kRsMaxSamples; }

extern "C" int vgan_rshash_build(const float* X, int ldx, int64_t n, int d, int first, int count, int T, int s, uint64_t seed,
                                 const int32_t* comp_dims, const int32_t* comp_feat, const double* comp_shift, const double* comp_width,
                                 uint64_t* cell_key, int32_t* cell_count, int32_t* n_cells, float* sample_min, float* sample_max,
                                 int32_t* sample_rows, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && comp_dims && comp_feat && comp_shift && comp_width && cell_key && cell_count && n_cells && sample_min && sample_max);
    VGAN_CHECK_ARG(d > 0 && ldx >= d && n >= 2 && n <= VGAN_RSHASH_MAX_ROWS && first >= 0 && count > 0);
    VGAN_CHECK_ARG(rshash_shape_ok(T, s) && s <= n && ((int64_t)first + count) * T <= 0x7FFFFFFFLL);
    const RsComponents comp = {comp_dims, comp_feat, comp_shift, comp_width};
    const RsState st = {(u64*)cell_key, cell_count, n_cells, sample_min, sample_max, sample_rows};
    hipLaunchKernelGGL(rshash_build_kernel, dim3((unsigned)(count * T)), dim3(kBlock), (size_t)rs_padded(s) * 12, (hipStream_t)stream, X, (long)ldx, (u64)n, d, first,
                       T, s, feistel_half_bits((u64)n), (u64)seed, comp, st);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_rshash_cell_sums(const float* Xq, int64_t row_stride, int64_t col_stride, int rows, int d, int64_t row_base, int first,
                                     int count, int T, int s, const int32_t* comp_dims, const int32_t* comp_feat, const double* comp_shift,
                                     const double* comp_width, const uint64_t* cell_key, const int32_t* cell_count, const int32_t* n_cells,
                                     const float* sample_min, const float* sample_max, const int32_t* sample_rows, const int64_t* table,
                                     int64_t* sums, int64_t ld_sums, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && comp_dims && comp_feat && comp_shift && comp_width && cell_key && cell_count && n_cells && sample_min && sample_max);
    VGAN_CHECK_ARG(table && sums && rows > 0 && d > 0 && row_base >= 0 && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG((col_stride == 1 && row_stride >= d) || (row_stride == 1 && col_stride >= rows));
    VGAN_CHECK_ARG(rshash_shape_ok(T, s) && ld_sums >= rows && ((int64_t)first + count) * T <= 0x7FFFFFFFLL);
    const RsComponents comp = {comp_dims, comp_feat, comp_shift, comp_width};
    const RsFitted st = {(const u64*)cell_key, cell_count, n_cells, sample_min, sample_max, sample_rows};
    // four rows a thread once that still leaves two workgroups for every CU of the 256
    const long blocks4 = ((long)rows + 4 * kBlock - 1) / (4 * kBlock), blocks1 = ((long)rows + kBlock - 1) / kBlock;
    const hipStream_t hs = (hipStream_t)stream;
    const bool wide = blocks4 * count >= 512;
    const dim3 grid((unsigned)(wide ? blocks4 : blocks1), count);
#define VGAN_RSHASH_LAUNCH(R, FIT)                                                                                                      \
    hipLaunchKernelGGL((rshash_sums_kernel<R, FIT>), grid, dim3(kBlock), (size_t)((s + 3) & ~3) * (FIT ? 14 : 10), hs, Xq, (long)row_stride, (long)col_stride, rows, d,       \
                       (long)row_base, first, T, s, comp, st, table, sums, (long)ld_sums)
    if (sample_rows) {
        if (wide) VGAN_RSHASH_LAUNCH(4, true);
        else VGAN_RSHASH_LAUNCH(1, true);
    } else {
        if (wide) VGAN_RSHASH_LAUNCH(4, false);
        else VGAN_RSHASH_LAUNCH(1, false);
    }
#undef VGAN_RSHASH_LAUNCH
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_rshash_scores(const int64_t* sums, int64_t ld_sums, int count, int rows, int64_t denom, float* score, int64_t ld_score,
                                  vgan_stream_t stream) {
    VGAN_CHECK_ARG(sums && score && count > 0 && count <= 65535 && rows > 0 && ld_sums >= rows && ld_score >= rows && denom > 0);
    hipLaunchKernelGGL(rshash_scores_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock), count), dim3(kBlock), 0, (hipStream_t)stream,
                       sums, (long)ld_sums, rows, (double)denom, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

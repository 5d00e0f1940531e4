// Outlier ensemble, after the detectors: per-subspace statistics of the finished score matrix [S, n] (float32), and the
// fused transform + combination of its rows (v-gan_amd/outlier.py: normalize / combination).
//
// Every kernel here sees a row of the matrix as kNChunk-element slices, slice b of row s in workgroup (b, s): a fixed
// partition that depends on n alone, so nothing below depends on how the detectors chunked or split their work.
//   moments  (zscore)  float64 partial sums per slice (thread order, wave butterfly, the four waves in order), one
//                      workgroup per row adds the slice partials in a fixed tree; two passes (sum, then squared deviations
//                      from the stored mean).  No float atomics.
//   extrema  (minmax)  the same shape with float min / max.
//   select   (robust)  segmented radix select, one 8-bit digit per pass, most significant first: the hist kernel counts the
//                      digit of every key that still matches the prefix found so far (LDS integer atomics, then one global
//                      integer add per non-empty bin and workgroup), the pick kernel scans the 256 counts of a row, takes
//                      the digit that holds the wanted rank and clears the counts.  Two ranks, (n - 1) / 2 and n / 2, are
//                      followed at once (they are equal for odd n); while their prefixes agree one histogram serves both.
//                      Median: 4 passes over order-preserving 32-bit keys of the float32 scores.  MAD: 8 passes over the
//                      bits of fabs(double(x) - centre), a non-negative float64 whose bits order like its value.
//                      Integer counts only: exact, and the same for every grid and arrival order.
//   combine            thread i walks the S rows in order: t = (double(x) - c_s) / w_s (IEEE subtract and divide), then
//                      sum_s p_s t or max_s t.
#include <math.h>

#include "vgan_common.hpp"

namespace vgan {

constexpr int kNPer = 16;                 // elements per thread of a slice
constexpr int kNChunk = kBlock * kNPer;   // elements per slice
constexpr double kMadToSigma = 0.6744897501960817;  // Phi^-1(3/4): scipy's median_abs_deviation(scale="normal")

struct SelectState {  // per row: the key prefixes found so far and the ranks left inside them
    unsigned long long prefix[2];
    unsigned rank[2];
    unsigned pad[2];
};
static_assert(sizeof(SelectState) == 32, "SelectState layout");

__device__ __forceinline__ unsigned f32_key(float x) {  // order-preserving: negative values flip all bits, others the sign
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_key(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// A thread's kNPer elements of a slice, all loads issued before the first use: indices past the end are clamped to the
// last element (an unconditional load; the callers mask those values or, for min / max, do not mind the repeat).
__device__ __forceinline__ void load_slice(const float* __restrict__ row, long base, int n, float (&x)[kNPer]) {
#pragma unroll
    for (int j = 0; j < kNPer; ++j) {
        const long i = base + (long)j * kBlock;
        x[j] = row[i < n ? i : (long)n - 1];
    }
}

// PASS 0: part[s, b] = sum of the slice; PASS 1: sum of (x - center[s])^2
template <int PASS>
__global__ __launch_bounds__(kBlock) void norm_moment_partial_kernel(const float* __restrict__ score, int ld, int n,
                                                                     const double* __restrict__ center, double* __restrict__ part) {
    __shared__ double red[4];
    const int s = blockIdx.y;
    const float* row = score + (long)s * ld;
    const long base = (long)blockIdx.x * kNChunk + threadIdx.x;
    const double c = PASS ? center[s] : 0.0;
    float x[kNPer];
    load_slice(row, base, n, x);
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < kNPer; ++j) {
        const double v = PASS ? ((double)x[j] - c) * ((double)x[j] - c) : (double)x[j];
        a += base + (long)j * kBlock < n ? v : 0.0;
    }
    a = block_sum(a, red);
    if (threadIdx.x == 0) part[(long)s * gridDim.x + blockIdx.x] = a;
}

// one workgroup per row: the slice partials in a fixed tree.  PASS 0: center = sum / n; PASS 1: scale = sqrt(sum / n), 0 -> 1
template <int PASS>
__global__ __launch_bounds__(kBlock) void norm_moment_final_kernel(const double* __restrict__ part, int nb, int n,
                                                                   double* __restrict__ center, double* __restrict__ scale) {
    __shared__ double red[4];
    const int s = blockIdx.x;
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += kBlock) a += part[(long)s * nb + b];
    a = block_sum(a, red);
    if (threadIdx.x == 0) {
        if (PASS) {
            const double w = sqrt(a / (double)n);
            scale[s] = w == 0.0 ? 1.0 : w;
        } else {
            center[s] = a / (double)n;
        }
    }
}

__global__ __launch_bounds__(kBlock) void norm_extrema_partial_kernel(const float* __restrict__ score, int ld, int n,
                                                                      float* __restrict__ part) {
    __shared__ float red[2][4];
    const int s = blockIdx.y;
    const float* row = score + (long)s * ld;
    const long base = (long)blockIdx.x * kNChunk + threadIdx.x;
    float x[kNPer];
    load_slice(row, base, n, x);
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int j = 0; j < kNPer; ++j) {
        lo = fminf(lo, x[j]);
        hi = fmaxf(hi, x[j]);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = lo, red[1][threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = part + 2 * ((long)s * gridDim.x + blockIdx.x);
        o[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        o[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}

__global__ __launch_bounds__(kBlock) void norm_extrema_final_kernel(const float* __restrict__ part, int nb, double* __restrict__ center,
                                                                    double* __restrict__ scale) {
    __shared__ float red[2][4];
    const int s = blockIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
        lo = fminf(lo, part[2 * ((long)s * nb + b)]);
        hi = fmaxf(hi, part[2 * ((long)s * nb + b) + 1]);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = lo, red[1][threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        const double w = (double)hi - (double)lo;
        center[s] = (double)lo;
        scale[s] = w == 0.0 ? 1.0 : w;
    }
}

// ---- segmented radix select ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void norm_select_init_kernel(SelectState* __restrict__ state, unsigned* __restrict__ hist, int S,
                                                                  int n) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    if (t < (long)S * 512) hist[t] = 0u;
    if (t < S) {
        SelectState st;
        st.prefix[0] = st.prefix[1] = 0ull;
        st.rank[0] = (unsigned)(n - 1) / 2u;
        st.rank[1] = (unsigned)n / 2u;
        st.pad[0] = st.pad[1] = 0u;
        state[t] = st;
    }
}

// counts digit (key >> shift) & 255 of the keys whose bits above shift + 8 equal the prefix (first pass: every key)
template <bool MAD>
__global__ __launch_bounds__(kBlock) void norm_select_hist_kernel(const float* __restrict__ score, int ld, int n,
                                                                  const double* __restrict__ center,
                                                                  const SelectState* __restrict__ state, unsigned* __restrict__ hist,
                                                                  int shift, int first_pass) {
    __shared__ unsigned bins[2][256];
    const int s = blockIdx.y;
    bins[0][threadIdx.x] = 0u;
    bins[1][threadIdx.x] = 0u;
    const SelectState st = state[s];
    const bool two = st.prefix[0] != st.prefix[1];
    const double c = MAD ? center[s] : 0.0;
    const float* row = score + (long)s * ld;
    const long base = (long)blockIdx.x * kNChunk + threadIdx.x;
    float x[kNPer];
    load_slice(row, base, n, x);
    __syncthreads();
    // bits above the digit; a shift by the full width is not defined, so the first pass skips the comparison
    const int up = first_pass ? 0 : shift + 8;
#pragma unroll
    for (int j = 0; j < kNPer; ++j) {
        const long i = base + (long)j * kBlock;
        if (i >= n) continue;
        const unsigned long long key =
            MAD ? (unsigned long long)__double_as_longlong(fabs((double)x[j] - c)) : (unsigned long long)f32_key(x[j]);
        const unsigned digit = (unsigned)(key >> shift) & 255u;
        if (first_pass || ((key ^ st.prefix[0]) >> up) == 0ull) atomicAdd(&bins[0][digit], 1u);
        if (two && ((key ^ st.prefix[1]) >> up) == 0ull) atomicAdd(&bins[1][digit], 1u);
    }
    __syncthreads();
    unsigned* h = hist + (long)s * 512;
    const unsigned c0 = bins[0][threadIdx.x], c1 = bins[1][threadIdx.x];
    if (c0) atomicAdd(&h[threadIdx.x], c0);
    if (c1) atomicAdd(&h[256 + threadIdx.x], c1);
}

// one workgroup per row: the digit that holds each rank joins its prefix; the counts are cleared for the next pass
__global__ __launch_bounds__(kBlock) void norm_select_pick_kernel(SelectState* __restrict__ state, unsigned* __restrict__ hist,
                                                                  int shift) {
    __shared__ unsigned scan[256];
    const int s = blockIdx.x, t = threadIdx.x;
    unsigned* h = hist + (long)s * 512;
    const SelectState st = state[s];
    const bool two = st.prefix[0] != st.prefix[1];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned cnt = h[(two ? r : 0) * 256 + t];
        scan[t] = cnt;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const unsigned add = t >= o ? scan[t - o] : 0u;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        const unsigned incl = scan[t], excl = incl - cnt;
        if (excl <= st.rank[r] && st.rank[r] < incl) {
            state[s].prefix[r] = st.prefix[r] | ((unsigned long long)t << shift);
            state[s].rank[r] = st.rank[r] - excl;
        }
        __syncthreads();
    }
    h[t] = 0u;
    h[256 + t] = 0u;
}

// the two selected keys of every row -> the median (MAD 0: center) or the scaled MAD (MAD 1: scale, 0 -> 1)
template <bool MAD>
__global__ void norm_select_final_kernel(const SelectState* __restrict__ state, int S, double* __restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const SelectState st = state[s];
    if (MAD) {
        const double a = __longlong_as_double((long long)st.prefix[0]), b = __longlong_as_double((long long)st.prefix[1]);
        const double w = (a + b) * 0.5 / kMadToSigma;
        out[s] = w == 0.0 ? 1.0 : w;
    } else {
        const double a = (double)f32_from_key((unsigned)st.prefix[0]), b = (double)f32_from_key((unsigned)st.prefix[1]);
        out[s] = (a + b) * 0.5;
    }
}

// unrolled so that the loads of eight rows are in flight before the first float64 divide needs one
template <bool MAX, bool NORM>
__global__ __launch_bounds__(256) void norm_combine_kernel(const float* __restrict__ score, int ld, int S, int n,
                                                           const double* __restrict__ center, const double* __restrict__ scale,
                                                           const double* __restrict__ p, double* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
#pragma unroll 8
    for (int s = 0; s < S; ++s) {
        double t = (double)score[(long)s * ld + i];
        if (NORM) t = (t - center[s]) / scale[s];
        if (MAX)
            a = (s == 0 || t > a) ? t : a;
        else
            a += p[s] * t;
    }
    out[i] = a;
}

static long norm_slices(int n) { return ((long)n + kNChunk - 1) / kNChunk; }

static int64_t norm_ws_bytes(int S, int n, int mode) {
    if (mode == VGAN_OUTLIER_NORM_ROBUST) return (int64_t)S * (sizeof(SelectState) + 512 * sizeof(unsigned));
    return (int64_t)S * norm_slices(n) * (int64_t)sizeof(double);  // one double, or two floats, per slice
}

template <bool MAD>
static int norm_select(const float* score, int ld, int S, int n, const double* center, SelectState* state, unsigned* hist,
                       double* out, hipStream_t st) {
    const dim3 grid((unsigned)norm_slices(n), S);
    hipLaunchKernelGGL(norm_select_init_kernel, dim3((S * 512 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, state, hist, S, n);
    VGAN_CHECK_LAUNCH();
    const int bits = MAD ? 64 : 32;
    for (int shift = bits - 8; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(norm_select_hist_kernel<MAD>, grid, dim3(kBlock), 0, st, score, ld, n, center, state, hist, shift,
                           shift == bits - 8 ? 1 : 0);
        VGAN_CHECK_LAUNCH();
        hipLaunchKernelGGL(norm_select_pick_kernel, dim3(S), dim3(kBlock), 0, st, state, hist, shift);
        VGAN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(norm_select_final_kernel<MAD>, dim3((S + 255) / 256), dim3(256), 0, st, state, S, out);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

}  // namespace vgan

using namespace vgan;

static bool norm_mode_ok(int mode) {
    return mode == VGAN_OUTLIER_NORM_ZSCORE || mode == VGAN_OUTLIER_NORM_ROBUST || mode == VGAN_OUTLIER_NORM_MINMAX;
}

extern "C" int64_t vgan_outlier_score_stats_ws_bytes(int S, int n, int mode) {
    if (!(S > 0 && S <= 65535 && n > 0 && norm_mode_ok(mode))) {
        set_error("%s:%d: bad argument: S > 0 && S <= 65535 && n > 0 && known mode", __FILE__, __LINE__);
        return -1;
    }
    return norm_ws_bytes(S, n, mode);
}

extern "C" int vgan_outlier_score_stats(const float* score, int ld, int S, int n, int mode, double* center, double* scale,
                                        void* workspace, int64_t workspace_bytes, vgan_stream_t stream) {
    VGAN_CHECK_ARG(score && center && scale && workspace && S > 0 && S <= 65535 && n > 0 && ld >= n);
    VGAN_CHECK_ARG(norm_mode_ok(mode));
    VGAN_CHECK_ARG(aligned16(workspace) && workspace_bytes >= norm_ws_bytes(S, n, mode));
    const hipStream_t st = (hipStream_t)stream;
    const int nb = (int)norm_slices(n);
    const dim3 grid(nb, S);
    if (mode == VGAN_OUTLIER_NORM_ZSCORE) {
        double* part = static_cast<double*>(workspace);
        hipLaunchKernelGGL(norm_moment_partial_kernel<0>, grid, dim3(kBlock), 0, st, score, ld, n, center, part);
        VGAN_CHECK_LAUNCH();
        hipLaunchKernelGGL(norm_moment_final_kernel<0>, dim3(S), dim3(kBlock), 0, st, part, nb, n, center, scale);
        VGAN_CHECK_LAUNCH();
        hipLaunchKernelGGL(norm_moment_partial_kernel<1>, grid, dim3(kBlock), 0, st, score, ld, n, center, part);
        VGAN_CHECK_LAUNCH();
        hipLaunchKernelGGL(norm_moment_final_kernel<1>, dim3(S), dim3(kBlock), 0, st, part, nb, n, center, scale);
        VGAN_CHECK_LAUNCH();
        return VGAN_OK;
    }
    if (mode == VGAN_OUTLIER_NORM_MINMAX) {
        float* part = static_cast<float*>(workspace);
        hipLaunchKernelGGL(norm_extrema_partial_kernel, grid, dim3(kBlock), 0, st, score, ld, n, part);
        VGAN_CHECK_LAUNCH();
        hipLaunchKernelGGL(norm_extrema_final_kernel, dim3(S), dim3(kBlock), 0, st, part, nb, center, scale);
        VGAN_CHECK_LAUNCH();
        return VGAN_OK;
    }
    SelectState* state = static_cast<SelectState*>(workspace);
    unsigned* hist = reinterpret_cast<unsigned*>(state + S);
    const int rc = norm_select<false>(score, ld, S, n, center, state, hist, center, st);
    if (rc != VGAN_OK) return rc;
    return norm_select<true>(score, ld, S, n, center, state, hist, scale, st);
}

extern "C" int vgan_outlier_combine_normalized(const float* score, int ld, int S, int n, const double* center, const double* scale,
                                               const double* weights, int combination, double* out, vgan_stream_t stream) {
    VGAN_CHECK_ARG(score && out && S > 0 && n > 0 && ld >= n);
    VGAN_CHECK_ARG((center == nullptr) == (scale == nullptr));
    VGAN_CHECK_ARG(combination == VGAN_OUTLIER_COMBINE_SUM || combination == VGAN_OUTLIER_COMBINE_MAX);
    VGAN_CHECK_ARG(combination == VGAN_OUTLIER_COMBINE_MAX || weights);
    const dim3 grid((unsigned)(((long)n + 255) / 256));
    const hipStream_t st = (hipStream_t)stream;
    const bool mx = combination == VGAN_OUTLIER_COMBINE_MAX;
    if (center)
        hipLaunchKernelGGL((mx ? norm_combine_kernel<true, true> : norm_combine_kernel<false, true>), grid, dim3(256), 0, st, score, ld, S,
                           n, center, scale, weights, out);
    else
        hipLaunchKernelGGL((mx ? norm_combine_kernel<true, false> : norm_combine_kernel<false, false>), grid, dim3(256), 0, st, score, ld,
                           S, n, center, scale, weights, out);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

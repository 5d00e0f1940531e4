// HiCS subspace contrast (Keller, Mueller, Boehm, ICDE 2012) for any list of feature sets: a Monte-Carlo sweep over
// (subspace, draw) pairs, all of it in integers (include/vgan_hip.h has the definition).
//
//   argsort  all d columns of X [n, d] at once: the bitonic network of outlier_ecod.hip on 64-bit keys (orderable float bits
//            << 32) | row.  The keys of a column are distinct, so the network's result is the stable order, ties to the lower
//            row.  A run of kHicsRun keys lives in LDS: the head launch sorts every run, then per merge size one launch for
//            each stride >= kHicsRun and one tail launch for the strides below it.  The last launch scatters order and rank.
//   draws    a group of kBlock / G threads owns one draw of one subspace; the G draws of a workgroup belong to the SAME
//            subspace, so every wave of the workgroup meets the same barriers.  The membership of the draw is a bitmap in
//            LDS indexed by the position in the comparison feature f_c:
//              2 w <= n   the first conditioning slice sets its w bits in map A (ds_or), every further one sets map B, which
//                         is ANDed into A.  alpha^(1 / (k - 1)) <= 1 / 2 holds only for a few features, so this loop is short;
//              2 w >  n   A starts full and every conditioning feature clears the n - w positions outside its slice
//                         (ds_and): the same set, (k - 1) (n - w) marks instead of (k - 1) w and no barrier between
//                         features, all (feature, position) pairs of the draw being dealt over the threads at once.
//            Then every thread takes a contiguous run of map words: popcounts, an exclusive scan over the group (wave
//            shuffles, the wave totals through LDS), and one walk over the bits of its words that follows cnt(r) n - r m in
//            64-bit integers through EVERY position r and keeps the largest magnitude.
//   sum      one thread per subspace adds D / (n m) over the draws in ascending order in float64.
#include "optim_common.hpp"

namespace vgan {

constexpr int kHicsRun = VGAN_HICS_SORT_RUN;  // keys of one LDS-resident run (16 KB)
constexpr int kHicsPairs = 4;                 // compare-exchanges per thread of a strided stage
constexpr int kHicsScratchWords = 16;         // per workgroup behind the maps: 4 wave counts, 4 wave maxima (64-bit)

__device__ __forceinline__ uint32_t hics_key(float v) {
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// position of compare-exchange t of a stage with stride j (a power of two): the lower index of the pair
__device__ __forceinline__ long hics_pair(long t, long j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// k_merge == 0 (head): keys from X, every stage of the merge sizes 2 .. run.  Otherwise (tail): keys from buf, the stages with
// stride run / 2 .. 1 of merge size k_merge.  last: the launch is the network's last, order and rank are written.
__global__ __launch_bounds__(kBlock) void hics_sort_local_kernel(const float* __restrict__ X, long ldx, int n, uint64_t* __restrict__ buf,
                                                                 long n_pad, int run, long k_merge, int last, uint32_t* __restrict__ order,
                                                                 uint32_t* __restrict__ rank) {
    __shared__ uint64_t key[kHicsRun];
    const long col = blockIdx.x, base = (long)blockIdx.y * run;
    uint64_t* out = buf + col * n_pad + base;
    for (int t = threadIdx.x; t < run; t += kBlock) {
        const long i = base + t;
        key[t] = k_merge == 0 ? (i < n ? ((uint64_t)hics_key(X[i * ldx + col]) << 32) | (uint64_t)i : ~0ull) : out[t];
    }
    __syncthreads();
    const long k_first = k_merge == 0 ? 2 : k_merge, k_last = k_merge == 0 ? run : k_merge;
    for (long k = k_first; k <= k_last; k <<= 1) {
        for (int j = (int)min(k >> 1, (long)(run >> 1)); j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (run >> 1); t += kBlock) {
                const int i = (int)hics_pair(t, j);
                const bool ascending = ((base + i) & k) == 0;
                const uint64_t a = key[i], b = key[i + j];
                if ((a > b) == ascending) {
                    key[i] = b;
                    key[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
    if (!last) {
        for (int t = threadIdx.x; t < run; t += kBlock) out[t] = key[t];
        return;
    }
    for (int t = threadIdx.x; t < run; t += kBlock) {
        const long r = base + t;
        if (r < n) {  // the pad keys are above every real key: the first n positions hold the n rows
            const uint32_t row = min((uint32_t)key[t], (uint32_t)(n - 1));
            order[col * n + r] = row;
            rank[col * n + row] = (uint32_t)r;
        }
    }
}

// one stage with stride j >= kHicsRun of merge size k; n_pad / 2 pairs a column, kHicsPairs a thread
__global__ __launch_bounds__(kBlock) void hics_sort_global_kernel(uint64_t* __restrict__ buf, long n_pad, long k, long j) {
    uint64_t* col = buf + (long)blockIdx.x * n_pad;
#pragma unroll
    for (int e = 0; e < kHicsPairs; ++e) {
        const long t = ((long)blockIdx.y * kHicsPairs + e) * kBlock + threadIdx.x;
        const long i = hics_pair(t, j);
        const bool ascending = (i & k) == 0;
        const uint64_t a = col[i], b = col[i + j];
        if ((a > b) == ascending) {
            col[i] = b;
            col[i + j] = a;
        }
    }
}

// word `word` of Philox block q of draw t
__device__ __forceinline__ unsigned hics_word(unsigned t, unsigned q, int word, unsigned k0, unsigned k1) {
    unsigned c[4] = {t, q, VGAN_HICS_PHILOX_TAG, 0u};
    philox4x32_10(c, k0, k1);
    return word == 0 ? c[0] : word == 1 ? c[1] : word == 2 ? c[2] : c[3];
}
__device__ __forceinline__ int hics_start(unsigned t, int p, int span, unsigned k0, unsigned k1) {
    return (int)(((unsigned long long)hics_word(t, 1u + ((unsigned)p >> 2), p & 3, k0, k1) * (unsigned long long)span) >> 32);
}

// G draws of one subspace per workgroup, kBlock / G threads each; blockIdx.x = subspace * groups + group of draws
template <int G>
__global__ __launch_bounds__(kBlock) void hics_contrast_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ rank, int n,
                                                               const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                               const int32_t* __restrict__ width, const uint64_t* __restrict__ stream_id,
                                                               int M, int groups, unsigned long long seed, int64_t* __restrict__ Dout,
                                                               int32_t* __restrict__ mout, int32_t* __restrict__ cout) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hics_lds[];
    constexpr int T = kBlock / G;      // threads of a draw
    constexpr int WAVES = T / kWave;   // waves of a draw
    const int z = blockIdx.x / groups, sub = threadIdx.x / T, tid = threadIdx.x % T, lane = threadIdx.x & 63;
    const int t = (blockIdx.x % groups) * G + sub;
    const bool live = t < M;
    const int f0 = feat_off[z], k = feat_off[z + 1] - f0;
    const long out = (long)z * M + t;
    if (k < 2) {  // the same for the whole workgroup
        if (live && tid == 0) {
            Dout[out] = 0;
            mout[out] = 0;
            cout[out] = -1;
        }
        return;
    }
    const int w = min(max(width[z], 1), n);
    const int nw = (n + 31) >> 5;
    uint32_t* A = hics_lds + (size_t)sub * 2 * nw;
    uint32_t* B = A + nw;
    uint32_t* scratch = hics_lds + (((size_t)G * 2 * nw + 3) & ~(size_t)3);
    int* wave_cnt = reinterpret_cast<int*>(scratch);                                      // [kBlock / kWave]
    unsigned long long* wave_best = reinterpret_cast<unsigned long long*>(scratch + 4);  // [kBlock / kWave]

    const unsigned long long id = stream_id[z];
    const unsigned k0 = (unsigned)seed ^ (unsigned)id, k1 = (unsigned)(seed >> 32) ^ (unsigned)(id >> 32) ^ 0x5bd1e995u;
    const int c = (int)(((unsigned long long)hics_word((unsigned)t, 0u, 0, k0, k1) * (unsigned long long)k) >> 32);
    const uint32_t* rank_c = rank + (long)feat[f0 + c] * n;
    const int span = n - w + 1;
    const uint32_t top = (uint32_t)(n - 1);

    if (2L * w <= n) {
        bool first = true;
        for (int p = 0; p < k; ++p) {
            if (p == c) continue;  // k - 1 turns for every draw of the workgroup, whatever its c
            uint32_t* map = first ? A : B;
            for (int i = tid; i < nw; i += T) map[i] = 0u;
            __syncthreads();
            if (live) {
                const uint32_t* ord = order + (long)feat[f0 + p] * n + hics_start((unsigned)t, p, span, k0, k1);
                for (int j = tid; j < w; j += T) {
                    const uint32_t pos = min(rank_c[min(ord[j], top)], top);
                    atomicOr(&map[pos >> 5], 1u << (pos & 31));
                }
            }
            __syncthreads();
            if (!first) {
                for (int i = tid; i < nw; i += T) A[i] &= B[i];
                __syncthreads();
            }
            first = false;
        }
    } else {
        const uint32_t tail = (n & 31) ? (1u << (n & 31)) - 1u : ~0u;
        for (int i = tid; i < nw; i += T) A[i] = i == nw - 1 ? tail : ~0u;
        __syncthreads();
        const int ex = n - w;  // positions of a feature outside its slice
        if (live && ex > 0) {
            const long total = (long)k * ex;
            for (long idx = tid; idx < total; idx += T) {
                const int p = (int)(idx / ex), e = (int)(idx - (long)p * ex);
                if (p == c) continue;
                const int start = hics_start((unsigned)t, p, span, k0, k1);
                const uint32_t row = order[(long)feat[f0 + p] * n + (e < start ? e : e + w)];
                const uint32_t pos = min(rank_c[min(row, top)], top);
                atomicAnd(&A[pos >> 5], ~(1u << (pos & 31)));
            }
        }
        __syncthreads();
    }

    // every thread: the words [i0, i1) of the map
    const int per = (nw + T - 1) / T;
    const int i0 = min(tid * per, nw), i1 = min(i0 + per, nw);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += __popc(A[i]);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_cnt[threadIdx.x >> 6] = incl;
    __syncthreads();
    const int wave0 = sub * WAVES, wave = threadIdx.x >> 6;
    int before = 0, m = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) {
        const int cnt = wave_cnt[wave0 + v];
        before += wave0 + v < wave ? cnt : 0;
        m += cnt;
    }
    // g(r) = cnt(r) n - r m, followed bit by bit from r = 32 i0
    const long long nn = n, mm = m, up = nn - mm;
    long long g = (long long)(before + incl - mine) * nn - (long long)i0 * 32 * mm;
    unsigned long long best = 0ull;
    for (int i = i0; i < i1; ++i) {
        const uint32_t word = A[i];
        const int bits = min(32, n - (i << 5));
        for (int b = 0; b < bits; ++b) {
            g += ((word >> b) & 1u) ? up : -mm;
            const unsigned long long mag = (unsigned long long)(g < 0 ? -g : g);
            best = mag > best ? mag : best;
        }
    }
    best = wave_max(best);
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    if (live && tid == 0) {
#pragma unroll
        for (int v = 0; v < WAVES; ++v) best = wave_best[wave0 + v] > best ? wave_best[wave0 + v] : best;
        Dout[out] = (int64_t)best;
        mout[out] = m;
        cout[out] = c;
    }
}

__global__ __launch_bounds__(kBlock) void hics_sum_kernel(const int64_t* __restrict__ D, const int32_t* __restrict__ m,
                                                          const int32_t* __restrict__ c, int n, int M, int S, double* __restrict__ contrast,
                                                          int32_t* __restrict__ n_empty) {
    const int z = blockIdx.x * kBlock + threadIdx.x;
    if (z >= S) return;
    double sum = 0.0;
    int empty = 0;
    for (int t = 0; t < M; ++t) {
        const long i = (long)z * M + t;
        const int mm = m[i];
        if (mm > 0)
            sum += (double)D[i] / (double)((long long)n * mm);
        else if (c[i] >= 0)
            ++empty;
    }
    contrast[z] = sum / (double)M;
    n_empty[z] = empty;
}

static size_t hics_lds_bytes(int n, int G) {
    const size_t nw = ((size_t)n + 31) >> 5;
    return ((((size_t)G * 2 * nw + 3) & ~(size_t)3) + kHicsScratchWords) * sizeof(uint32_t);
}

// lets the draw kernels take the two maps of VGAN_HICS_MAX_ROWS rows and the scratch words behind them
template <class Kernel>
static int hics_allow_lds(Kernel kernel) {
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)hics_lds_bytes(VGAN_HICS_MAX_ROWS, 1));
    if (attr != hipSuccess) {
        set_error("%s:%d: hipFuncSetAttribute failed: %s", __FILE__, __LINE__, hipGetErrorString(attr));
        return VGAN_ERR_HIP;
    }
    return VGAN_OK;
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_hics_argsort_columns(const float* X, int ldx, int n, int d, uint64_t* keys, int64_t n_pad, uint32_t* order,
                                         uint32_t* rank, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && keys && order && rank && d > 0 && ldx >= d && n >= 2 && n <= VGAN_HICS_MAX_ROWS);
    VGAN_CHECK_ARG(n_pad >= n && (n_pad & (n_pad - 1)) == 0 && n_pad < 2 * (int64_t)n);
    const hipStream_t st = (hipStream_t)stream;
    const int run = (int)(n_pad < kHicsRun ? n_pad : kHicsRun);
    const dim3 local(d, (unsigned)(n_pad / run));
    hipLaunchKernelGGL(hics_sort_local_kernel, local, dim3(kBlock), 0, st, X, (long)ldx, n, keys, (long)n_pad, run, 0L,
                       n_pad == run ? 1 : 0, order, rank);
    VGAN_CHECK_LAUNCH();
    for (long k = 2L * run; k <= n_pad; k <<= 1) {
        const dim3 strided(d, (unsigned)(n_pad / 2 / (kHicsPairs * kBlock)));
        for (long j = k >> 1; j >= run; j >>= 1)
            hipLaunchKernelGGL(hics_sort_global_kernel, strided, dim3(kBlock), 0, st, keys, (long)n_pad, k, j);
        hipLaunchKernelGGL(hics_sort_local_kernel, local, dim3(kBlock), 0, st, X, (long)ldx, n, keys, (long)n_pad, run, k,
                           k == n_pad ? 1 : 0, order, rank);
        VGAN_CHECK_LAUNCH();
    }
    return VGAN_OK;
}

extern "C" int vgan_hics_contrast(const uint32_t* order, const uint32_t* rank, int n, int d, const int32_t* feat, const int32_t* feat_off,
                                  const int32_t* width, const uint64_t* stream_id, int S, int M, uint64_t seed, int group, int64_t* D,
                                  int32_t* m, int32_t* c, double* contrast, int32_t* n_empty, vgan_stream_t stream) {
    VGAN_CHECK_ARG(order && rank && feat && feat_off && width && stream_id && D && m && c && contrast && n_empty);
    VGAN_CHECK_ARG(n >= 2 && n <= VGAN_HICS_MAX_ROWS && d > 0 && S > 0 && M > 0);
    VGAN_CHECK_ARG(group == 0 || group == 1 || group == VGAN_HICS_WAVE_GROUP);
    VGAN_CHECK_ARG(group != VGAN_HICS_WAVE_GROUP || n <= VGAN_HICS_WAVE_GROUP_MAX_ROWS);
    // a wave per draw up to 2^14 rows, a workgroup per draw beyond: measured on all pairs of 64 features, 50 draws, the wave
    // shape takes 0.72 / 0.98 / 1.12 / 1.81 of the workgroup shape's time at n = 4096 / 16384 / 32768 / 65536
    const int G = group ? group : (n <= 16384 ? VGAN_HICS_WAVE_GROUP : 1);
    const int groups = (M + G - 1) / G;
    VGAN_CHECK_ARG((int64_t)S * groups <= 2147483647LL);
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = hics_lds_bytes(n, G);
    const dim3 grid((unsigned)((int64_t)S * groups));
    if (G == 1) {
        if (lds > 65536) {
            static const int allowed = hics_allow_lds(&hics_contrast_kernel<1>);
            if (allowed != VGAN_OK) return allowed;
        }
        hipLaunchKernelGGL(hics_contrast_kernel<1>, grid, dim3(kBlock), lds, st, order, rank, n, feat, feat_off, width, stream_id, M,
                           groups, (unsigned long long)seed, D, m, c);
    } else {
        if (lds > 65536) {
            static const int allowed = hics_allow_lds(&hics_contrast_kernel<VGAN_HICS_WAVE_GROUP>);
            if (allowed != VGAN_OK) return allowed;
        }
        hipLaunchKernelGGL(hics_contrast_kernel<VGAN_HICS_WAVE_GROUP>, grid, dim3(kBlock), lds, st, order, rank, n, feat, feat_off, width,
                           stream_id, M, groups, (unsigned long long)seed, D, m, c);
    }
    VGAN_CHECK_LAUNCH();
    hipLaunchKernelGGL(hics_sum_kernel, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, st, D, m, c, n, M, S, contrast, n_empty);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

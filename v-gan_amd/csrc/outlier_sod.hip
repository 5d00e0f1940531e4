// Subspace outlier degree (SOD: Kriegel, Kroeger, Schubert, Zimek 2009; pyod's SOD) over the refined neighbour lists of
// outlier.hip.  Per subspace s (features F_s ascending, d_s of them), with N(j) the fit-time list of fitted row j (self
// excluded) and N(x) the list of the row x that is scored (a fitted row's own list at fit, a new row's list with nothing
// excluded afterwards):
//   SNN(x, j) = |N(x) n N(j)| for every fitted j (j != x at fit)
//   R(x)      = the first ref_set fitted rows in the order (SNN descending, row index ascending); rows with SNN = 0 take part
//   mu_f, v_f = mean and population variance of feature f over R(x), float64 from the raw float32 values, the rows in the
//               order of R, every difference, square, sum and quotient rounded on its own (no fma)
//   V = sum_f v_f, T = (alpha V) / d_s, f is relevant iff v_f < T, r = the number of relevant features
//   Q = sum over the relevant f of (x_f - mu_f)^2;  score = sqrt(Q / r) (pyod) or sqrt(Q) / r (paper), 0 where r = 0
// V and Q are summed in one shape: lane l of 64 adds its features l, l + 64, ... (positions in F_s) in ascending order,
// then the 64 partial sums are added in lane order.
//
// Reverse lists.  SNN(x, .) is a sparse integer product: for m in N(x), for j in RN(m) = {j : m in N(j)}, count[j] += 1.
// RN is a CSR per subspace built from the fit-time lists by an integer count (global atomics), an exclusive scan per
// subspace and a fill through an atomic cursor.  The order of the rows inside one RN(m) depends on the launch and does not
// matter: only integer counts are formed from it.
//
// Reference sets.  One wave (a 64-thread workgroup) works through query rows of one subspace.  The counts of all fitted rows
// sit in LDS as packed bytes, four rows a word (SNN <= 32, so no byte carries), incremented with 32-bit LDS atomics.  That
// table bounds VGAN_SOD_MAX_ROWS: 2^15 rows are 32 KiB, which leaves four workgroups a CU; up to 2^13 and 2^14 rows the 8 KiB
// and 16 KiB instantiations run.  (One workgroup may hold 160 KiB, which would carry 2^17 rows at one wave a CU: not built.)
// Lane l owns a contiguous power-of-two run of table words, so lane order then word order then byte order is row order.
// An increment whose byte was 0 marks its word (or group of up to four words) in the lane's 32-bit dirty mask; the
// selection and the clearing walk only marked words.  Selection: a histogram of the touched counts, then
// level by level from k down over the levels that are not empty: every lane counts its rows of the level, a wave prefix sum
// gives their places, and they are written until ref_set is full.  What is still missing after level 1 is taken from the
// rows with count 0 in ascending order (a ballot over 64 rows at a time); such a query row is `unshared`.
//
// Scores.  One wave per (subspace, row), four a workgroup, lanes over the positions of F_s.  The moments of a feature are
// formed twice, once for V and once for the mask and Q: v_f of up to 8192 features has no place in registers, and the second
// gather reads what the first one left in the caches.  Both passes run the same instructions, so v_f is the same value.
#include "vgan_common.hpp"

namespace vgan {

constexpr int kSodWave = 64;                 // threads of a reference-set workgroup
constexpr int kSodLevels = VGAN_OUTLIER_MAX_K + 1;
constexpr int kSodScoreWaves = kBlock / kWave;

// cnt[z, m] += 1 for every entry m of the lists idx [count, n, k]
__global__ __launch_bounds__(kBlock) void sod_count_kernel(const int32_t* __restrict__ idx, long total, int n, int k,
                                                          int32_t* __restrict__ cnt) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const long z = i / ((long)n * k);
    const int m = idx[i];
    if ((unsigned)m < (unsigned)n) atomicAdd(&cnt[z * n + m], 1);
}

// One workgroup per subspace: off[z, 0 .. n] = the exclusive prefix sums of cnt[z, .], which are also left in cnt as the
// cursors of the fill.  n <= VGAN_SOD_MAX_ROWS: a thread owns at most 128 consecutive rows.
__global__ __launch_bounds__(kBlock) void sod_scan_kernel(int32_t* __restrict__ cnt, int n, int32_t* __restrict__ off) {
    __shared__ int part[kBlock];
    const int z = blockIdx.x, tid = threadIdx.x;
    int32_t* c = cnt + (long)z * n;
    int32_t* o = off + (long)z * (n + 1);
    const int per = (n + kBlock - 1) / kBlock;
    const int b = min(tid * per, n), e = min(b + per, n);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += c[i];
    part[tid] = sum;
    __syncthreads();
    for (int s = 1; s < kBlock; s <<= 1) {
        const int v = tid >= s ? part[tid - s] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int i = b; i < e; ++i) {
        const int c0 = c[i];
        o[i] = run;
        c[i] = run;
        run += c0;
    }
    if (tid == kBlock - 1) o[n] = part[kBlock - 1];
}

// rows[z, cursor[z, m]++] = x for every entry m of the list of row x
__global__ __launch_bounds__(kBlock) void sod_fill_kernel(const int32_t* __restrict__ idx, long total, int n, int k,
                                                         int32_t* __restrict__ cursor, int32_t* __restrict__ rows) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const long nk = (long)n * k;
    const long z = i / nk;
    const int x = (int)((i - z * nk) / k);
    const int m = idx[i];
    if ((unsigned)m >= (unsigned)n) return;
    const int pos = atomicAdd(&cursor[z * n + m], 1);
    if ((unsigned)pos < (unsigned)nk) rows[z * nk + pos] = x;
}

template <int TW>  // words of the count table: 4 TW rows
__global__ __launch_bounds__(kSodWave) void sod_refset_kernel(const int32_t* __restrict__ idxq, int nq,
                                                             const int32_t* __restrict__ rn_off,
                                                             const int32_t* __restrict__ rn_rows, int nr, int k, int ref_set,
                                                             int exclude_self, int32_t* __restrict__ refset,
                                                             int32_t* __restrict__ n_unshared) {
    __shared__ unsigned tab[TW];
    __shared__ unsigned dirty[kSodWave];
    __shared__ int hist[kSodLevels];
    __shared__ int lst[VGAN_OUTLIER_MAX_K];
    const int lane = threadIdx.x, z = blockIdx.y;
    // lane l owns the words [l << lw, (l + 1) << lw); a bit of its dirty mask covers 1 << lg of them
    const int nwords = (nr + 3) >> 2;
    int lw = 0;
    while ((kSodWave << lw) < nwords) ++lw;
    const int lg = lw > 5 ? lw - 5 : 0;
    const int wbase = lane << lw, wmask = (1 << lw) - 1;
    for (int w = lane; w < TW; w += kSodWave) tab[w] = 0u;
    dirty[lane] = 0u;
    if (lane < kSodLevels) hist[lane] = 0;
    __syncthreads();

    const int32_t* off = rn_off + (long)z * (nr + 1);
    const long nk = (long)nr * k;
    const int32_t* rows = rn_rows + (long)z * nk;

    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int self = exclude_self ? q : -1;
        if (lane < k) {
            const int m = idxq[((long)z * nq + q) * k + lane];
            lst[lane] = (unsigned)m < (unsigned)nr ? m : -1;
        }
        __syncthreads();

        // count[j] += 1 for j in RN(m), m in N(q); the first touch of a byte marks its word
        for (int a = 0; a < k; ++a) {
            const int m = lst[a];
            if (m < 0) continue;
            const long b = max(off[m], 0), e = min((long)off[m + 1], nk);
            for (long p = b + lane; p < e; p += kSodWave) {
                const int j = rows[p];
                if ((unsigned)j >= (unsigned)nr) continue;
                const int w = j >> 2, sh = (j & 3) * 8;
                const unsigned old = atomicAdd(&tab[w], 1u << sh);
                if (((old >> sh) & 0xffu) == 0u) atomicOr(&dirty[w >> lw], 1u << ((w & wmask) >> lg));
            }
        }
        __syncthreads();

        // f(row, count) for the touched rows of this lane except q itself, rows ascending
        const unsigned dm = dirty[lane];
        auto walk = [&](auto&& f) {
            for (unsigned bits = dm; bits; bits &= bits - 1u) {
                const int g = __ffs((int)bits) - 1;
                const int w0 = wbase + (g << lg);
                for (int w = w0; w < w0 + (1 << lg); ++w) {
                    const unsigned v = tab[w];
                    if (!v) continue;
#pragma unroll
                    for (int b4 = 0; b4 < 4; ++b4) {
                        const int c = (int)((v >> (8 * b4)) & 0xffu);
                        if (c && 4 * w + b4 != self) f(4 * w + b4, c);
                    }
                }
            }
        };
        walk([&](int, int c) { atomicAdd(&hist[min(c, kSodLevels - 1)], 1); });
        __syncthreads();

        int32_t* out = refset + ((long)z * nq + q) * ref_set;
        int filled = 0;
        for (int c = k; c >= 1 && filled < ref_set; --c) {
            const int hc = hist[c];
            if (!hc) continue;
            int mine = 0;
            walk([&](int, int cj) { mine += cj == c; });
            int incl = mine;
#pragma unroll
            for (int o = 1; o < kSodWave; o <<= 1) {
                const int t = __shfl_up(incl, o, kSodWave);
                if (lane >= o) incl += t;
            }
            int pos = filled + incl - mine;
            if (mine && pos < ref_set)
                walk([&](int j, int cj) {
                    if (cj == c) {
                        if (pos < ref_set) out[pos] = j;
                        ++pos;
                    }
                });
            filled += hc;
        }
        if (filled < ref_set) {
            // the tail: rows that share nothing with q, ascending
            if (n_unshared && lane == 0) atomicAdd(&n_unshared[z], 1);
            for (int base = 0; base < nr && filled < ref_set; base += kSodWave) {
                const int j = base + lane;
                const bool zero = j < nr && j != self && ((tab[j >> 2] >> ((j & 3) * 8)) & 0xffu) == 0u;
                const unsigned long long bal = __ballot(zero);
                const int pos = filled + __popcll(bal & ((1ull << lane) - 1ull));
                if (zero && pos < ref_set) out[pos] = j;
                filled += __popcll(bal);
            }
            for (int p = filled + lane; p < ref_set; p += kSodWave) out[p] = -1;  // ref_set > the rows there are: refused by the host
        }
        __syncthreads();

        // clear what was touched
        for (unsigned bits = dm; bits; bits &= bits - 1u) {
            const int w0 = wbase + ((__ffs((int)bits) - 1) << lg);
            for (int w = w0; w < w0 + (1 << lg); ++w) tab[w] = 0u;
        }
        dirty[lane] = 0u;
        if (lane < kSodLevels) hist[lane] = 0;
        __syncthreads();
    }
}

// the 64 partial sums in lane order; every lane of the wave is active
__device__ __forceinline__ double sod_lane_order_sum(double p) {
    double tot = 0.0;
    for (int l = 0; l < kWave; ++l) tot += __shfl(p, l, kWave);
    return tot;
}

__global__ __launch_bounds__(kBlock) void sod_score_kernel(const float* __restrict__ Xq, int ldq, int nq,
                                                          const float* __restrict__ Xr, int ldr, int nr,
                                                          const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                          int first, const int32_t* __restrict__ refset, int ref_set, double alpha,
                                                          int form, float* __restrict__ score, const int32_t* __restrict__ score_row,
                                                          int ld_score, int32_t* __restrict__ n_relevant,
                                                          uint32_t* __restrict__ mask, int mask_words) {
    __shared__ int lds_ref[kSodScoreWaves][kWave];
    const int z = blockIdx.y, s = first + z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q_raw = blockIdx.x * kSodScoreWaves + wave;
    const int q = min(q_raw, nq - 1);  // a surplus wave repeats the last row and stores nothing
    const int f0 = feat_off[s], ds = feat_off[s + 1] - f0;
    {
        const int r = lane < ref_set ? refset[((long)z * nq + q) * ref_set + lane] : -1;
        lds_ref[wave][lane] = (unsigned)r < (unsigned)nr ? r : -1;  // an entry outside the fitted rows counts as the origin
    }
    __syncthreads();
    const int* ref = lds_ref[wave];
    const float* xq = Xq + (long)q * ldq;
    const double rs = (double)ref_set;

    auto moments = [&](int f, double& mu, double& v) {
        double s1 = 0.0;
        for (int r = 0; r < ref_set; ++r) {
            const int row = ref[r];
            s1 += row >= 0 ? (double)Xr[(long)row * ldr + f] : 0.0;
        }
        mu = s1 / rs;
        double s2 = 0.0;
        for (int r = 0; r < ref_set; ++r) {
            const int row = ref[r];
            const double dlt = (row >= 0 ? (double)Xr[(long)row * ldr + f] : 0.0) - mu;
            s2 += mul_rounded_free(dlt, dlt);
        }
        v = s2 / rs;
    };

    // every lane runs every trip (the sums below shuffle over the whole wave); a lane past d_s repeats the last feature
    const int trips = (ds + kWave - 1) / kWave;
    double pv = 0.0;
    for (int t = 0; t < trips; ++t) {
        const int i = t * kWave + lane;
        double mu, v;
        moments(feat[f0 + min(i, ds - 1)], mu, v);
        if (i < ds) pv += v;
    }
    const double V = sod_lane_order_sum(pv);
    const double thr = mul_rounded_free(alpha, V) / (double)ds;

    double pq = 0.0;
    int r = 0;
    uint32_t* mrow = mask ? mask + ((long)z * nq + q) * mask_words : nullptr;
    for (int t = 0; t < trips; ++t) {
        const int i = t * kWave + lane;
        const int f = feat[f0 + min(i, ds - 1)];
        double mu, v;
        moments(f, mu, v);
        const double dq = (double)xq[f] - mu;
        const double sq = mul_rounded_free(dq, dq);
        const bool rel = i < ds && v < thr;
        if (rel) pq += sq;
        const unsigned long long bal = __ballot(rel);
        r += __popcll(bal);
        if (mrow && q_raw < nq && lane < 2 && 2 * t + lane < mask_words) mrow[2 * t + lane] = (uint32_t)(bal >> (32 * lane));
    }
    const double Q = sod_lane_order_sum(pq);
    double val = 0.0;
    if (r > 0) val = form == VGAN_SOD_FORM_PAPER ? sqrt(Q) / (double)r : sqrt(Q / (double)r);
    if (lane == 0 && q_raw < nq) {
        score[(long)(score_row ? score_row[z] : z) * ld_score + q] = (float)val;
        n_relevant[(long)z * nq + q] = r;
    }
}

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_sod_reverse_lists(const int32_t* idx, int n, int k, int count, int32_t* rn_off, int32_t* rn_rows,
                                      int32_t* cursor, vgan_stream_t stream) {
    VGAN_CHECK_ARG(idx && rn_off && rn_rows && cursor && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(k >= 1 && k <= VGAN_OUTLIER_MAX_K && n > k && n <= VGAN_SOD_MAX_ROWS);
    const hipStream_t st = (hipStream_t)stream;
    const long total = (long)count * n * k;
    const unsigned blocks = (unsigned)((total + kBlock - 1) / kBlock);
    if (hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)count * n, st) != hipSuccess) {
        set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        return VGAN_ERR_HIP;
    }
    hipLaunchKernelGGL(sod_count_kernel, dim3(blocks), dim3(kBlock), 0, st, idx, total, n, k, cursor);
    hipLaunchKernelGGL(sod_scan_kernel, dim3(count), dim3(kBlock), 0, st, cursor, n, rn_off);
    hipLaunchKernelGGL(sod_fill_kernel, dim3(blocks), dim3(kBlock), 0, st, idx, total, n, k, cursor, rn_rows);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_sod_reference_sets(const int32_t* idxq, int nq, const int32_t* rn_off, const int32_t* rn_rows, int nr, int k,
                                       int count, int ref_set, int exclude_self, int32_t* refset, int32_t* n_unshared,
                                       vgan_stream_t stream) {
    VGAN_CHECK_ARG(idxq && rn_off && rn_rows && refset && nq > 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(k >= 1 && k <= VGAN_OUTLIER_MAX_K && nr > k && nr <= VGAN_SOD_MAX_ROWS);
    VGAN_CHECK_ARG(ref_set >= 1 && ref_set <= VGAN_SOD_MAX_REF && ref_set <= nr - (exclude_self ? 1 : 0));
    VGAN_CHECK_ARG(!exclude_self || nq == nr);
    const hipStream_t st = (hipStream_t)stream;
    if (n_unshared && hipMemsetAsync(n_unshared, 0, sizeof(int32_t) * (size_t)count, st) != hipSuccess) {
        set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        return VGAN_ERR_HIP;
    }
    // enough workgroups to fill the chip five deep; each walks its query rows with stride gridDim.x
    const int bx = min(nq, max(64, (8192 + count - 1) / count));
    const dim3 grid(bx, count);
    if (nr <= VGAN_SOD_MAX_ROWS / 4)
        hipLaunchKernelGGL((sod_refset_kernel<VGAN_SOD_MAX_ROWS / 16>), grid, dim3(kSodWave), 0, st, idxq, nq, rn_off, rn_rows, nr, k,
                           ref_set, exclude_self ? 1 : 0, refset, n_unshared);
    else if (nr <= VGAN_SOD_MAX_ROWS / 2)
        hipLaunchKernelGGL((sod_refset_kernel<VGAN_SOD_MAX_ROWS / 8>), grid, dim3(kSodWave), 0, st, idxq, nq, rn_off, rn_rows, nr, k,
                           ref_set, exclude_self ? 1 : 0, refset, n_unshared);
    else
        hipLaunchKernelGGL((sod_refset_kernel<VGAN_SOD_MAX_ROWS / 4>), grid, dim3(kSodWave), 0, st, idxq, nq, rn_off, rn_rows, nr, k,
                           ref_set, exclude_self ? 1 : 0, refset, n_unshared);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_sod_score(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                              const int32_t* feat_off, int first, int count, const int32_t* refset, int ref_set, double alpha,
                              int form, float* score, const int32_t* score_row, int ld_score, int32_t* n_relevant, uint32_t* mask,
                              int mask_words, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && Xr && feat && feat_off && refset && score && n_relevant && nq > 0 && nr > 0 && d > 0);
    VGAN_CHECK_ARG(ldq >= d && ldr >= d && first >= 0 && count > 0 && count <= 65535 && ld_score >= nq);
    VGAN_CHECK_ARG(ref_set >= 1 && ref_set <= VGAN_SOD_MAX_REF && alpha > 0.0 && alpha <= 1.0);
    VGAN_CHECK_ARG(form == VGAN_SOD_FORM_PYOD || form == VGAN_SOD_FORM_PAPER);
    VGAN_CHECK_ARG(!mask || mask_words > 0);
    hipLaunchKernelGGL(sod_score_kernel, dim3((nq + kSodScoreWaves - 1) / kSodScoreWaves, count), dim3(kBlock), 0, (hipStream_t)stream,
                       Xq, ldq, nq, Xr, ldr, nr, feat, feat_off, first, refset, ref_set, alpha, form, score, score_row, ld_score,
                       n_relevant, mask, mask_words);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

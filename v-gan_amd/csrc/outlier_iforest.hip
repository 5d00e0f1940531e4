// Isolation forest (Liu, Ting, Zhou 2008; sklearn's IsolationForest, pyod's IForest) over the subspaces: T random trees per
// subspace on psi sampled rows each, and per query row the sum of its path lengths through them.  Nothing here is n x n:
// the build touches psi rows per tree, scoring is a walk of at most L = ceil(log2 psi) steps per (row, tree).
//
//   trees    heap-numbered (root 1, children 2 i and 2 i + 1, slot 0 unused), N = 2^(L + 1) slots of 8 bytes a tree, [S, T, N]:
//            word 0 = the split feature (a column of X), -1 for a leaf, -2 for an absent slot; word 1 = the float32 threshold
//            of an internal node, the number of sample rows of a leaf, 0 where absent.  A row goes left iff x <= threshold.
//   build    one workgroup per tree.  The psi sampled row indices (feistel_perm of the tree's stream) live in LDS and are
//            partitioned level by level between two LDS arrays; a level's nodes are dealt to the four waves, one barrier per
//            level.  Per node a wave takes the float32 min and max of every feature of the subspace over the node's rows
//            (lanes over features, a loop over rows: consecutive features are neighbouring addresses of one row), counts the
//            non-constant ones, draws the Philox words of the node, takes min and max of the chosen feature again over the
//            rows (lanes over rows), forms the threshold in float64 with separately rounded operations and partitions the
//            rows (left from the front, right from the back of the node's segment: only the row sets matter).  The tree is
//            assembled in LDS and stored once, coalesced.  Loads: about psi d_s L per tree, from at most psi rows.
//   sums     a workgroup owns one subspace and kIfRowsPerThread x kBlock query rows; it stages the subspace's trees through
//            LDS a group at a time (as many as fit in kIfGroupBytes) and walks its rows through each, R rows a thread
//            interleaved for independent loads.  One 8-byte LDS read and one element gather Xq[row, feature] (row-major, as
//            given) per step; the depth of the leaf is read off its heap number.  A row's contribution (depth << 32) +
//            cq[size] is an integer, so the int64 total does not depend on any order or grouping.
//   scores   float32(exp2(-(double(sum) / double(denom)))), denom = T cq[psi].
//   blocks   vgan_iforest_build_blocks / vgan_iforest_path_sums_blocks run the same two kernels on one matrix PER BLOCK
//            (SubspaceDIF: block b grows its trees on its own representation R[b], [n, q], every column a candidate): the
//            matrix of block b starts block_stride elements after that of block b - 1 and there is no feature table (feat
//            NULL: the features are the columns 0 .. q - 1).  The subspace entries pass block_stride = 0 and their table.
#include "optim_common.hpp"
#include "vgan_common.hpp"

namespace vgan {

constexpr int kIfMaxSamples = VGAN_IFOREST_MAX_SAMPLES;    // psi
constexpr int kIfMaxSlots = 2 * kIfMaxSamples;             // N at psi = kIfMaxSamples
constexpr int kIfMaxDims = VGAN_IFOREST_MAX_DIMS;          // features of one subspace
constexpr int kIfWaves = kBlock / kWave;
constexpr int kIfGroupBytes = 32768;                       // LDS of one staged group of trees
constexpr int kIfGroupSlots = kIfGroupBytes / 8;
constexpr int kIfAbsent = 0xFFFF;                          // count of a slot no row can reach
constexpr unsigned kIfPhiloxTag = 0x49464F52u;             // "IFOR": counter word 2 of every draw

__device__ __forceinline__ float if_value(float v) { return v == 0.f ? 0.f : v; }  // -0.0 as +0.0

__device__ __forceinline__ float if_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(kBlock) void iforest_build_kernel(const float* __restrict__ X, long ldx, unsigned long long n,
                                                               const int32_t* __restrict__ feat, const int32_t* __restrict__ feat_off,
                                                               int first, int T, int psi, int L, int w, unsigned long long seed,
                                                               int2* __restrict__ nodes, long block_stride, int block_cols) {
    __shared__ int rows[2][kIfMaxSamples];
    __shared__ int2 tree[kIfMaxSlots];
    __shared__ unsigned short seg_start[kIfMaxSlots], seg_count[kIfMaxSlots];
    __shared__ unsigned long long varying[kIfWaves][kIfMaxDims / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = first + (int)(blockIdx.x / (unsigned)T), t = (int)(blockIdx.x % (unsigned)T);
    const unsigned long long id = (unsigned long long)s * (unsigned long long)T + (unsigned long long)t;
    const int N = 2 << L;
    // feat NULL: block s reads its own matrix of block_cols columns, all of them candidates
    const int off = feat ? feat_off[s] : 0, ds = feat ? min(feat_off[s + 1] - off, kIfMaxDims) : block_cols;
    X += (long)(s - first) * block_stride;
    const unsigned k0 = (unsigned)seed ^ (unsigned)id, k1 = (unsigned)(seed >> 32) ^ (unsigned)(id >> 32) ^ 0x5bd1e995u;

    for (int i = tid; i < psi; i += kBlock) rows[0][i] = (int)feistel_perm((unsigned long long)i, n, w, seed, id);
    for (int i = tid; i < N; i += kBlock) {
        tree[i] = make_int2(-2, 0);
        seg_start[i] = 0;
        seg_count[i] = (unsigned short)(i == 1 ? psi : kIfAbsent);
    }
    __syncthreads();

    for (int e = 0; e <= L; ++e) {
        const int* src = rows[e & 1];
        int* dst = rows[(e & 1) ^ 1];
        for (int node = (1 << e) + wave; node < (2 << e); node += kIfWaves) {
            const int m = seg_count[node];
            if (m == kIfAbsent) continue;  // the same for the whole wave
            const int s0 = seg_start[node];
            int c = 0;
            if (m > 1 && e < L) {
                for (int q = 0; q * 64 < ds; ++q) {
                    const int f = q * 64 + lane;
                    const long col = f < ds ? (feat ? feat[off + f] : f) : 0;
                    float lo = INFINITY, hi = -INFINITY;
                    if (f < ds)
                        for (int r = 0; r < m; ++r) {
                            const float x = if_value(X[(long)src[s0 + r] * ldx + col]);
                            lo = fminf(lo, x);
                            hi = fmaxf(hi, x);
                        }
                    const unsigned long long mask = __ballot(f < ds && lo != hi);
                    if (lane == 0) varying[wave][q] = mask;
                    c += __popcll(mask);
                }
                __builtin_amdgcn_wave_barrier();  // this wave's own LDS stores above are read back below
            }
            if (c == 0) {
                if (lane == 0) tree[node] = make_int2(-1, m);
                continue;
            }
            unsigned ctr[4] = {(unsigned)node, 0u, kIfPhiloxTag, 0u};
            philox4x32_10(ctr, k0, k1);
            int j = (int)(((unsigned long long)ctr[0] * (unsigned long long)c) >> 32);
            int q = 0;
            unsigned long long mask = varying[wave][0];
            while (j >= __popcll(mask)) {  // ends: the masks hold c > j bits in all
                j -= __popcll(mask);
                mask = varying[wave][++q];
            }
            for (; j > 0; --j) mask &= mask - 1;
            const int pos = q * 64 + (__ffsll((long long)mask) - 1);
            const long col = feat ? feat[off + pos] : pos;
            float lo = INFINITY, hi = -INFINITY;
            for (int r = lane; r < m; r += 64) {
                const float x = if_value(X[(long)src[s0 + r] * ldx + col]);
                lo = fminf(lo, x);
                hi = fmaxf(hi, x);
            }
            lo = if_wave_min(lo);
            hi = wave_max(hi);
            // three separately rounded float64 operations (mul_rounded: the sum must not absorb the product)
            const double u = ((double)ctr[1] + 0.5) * 0x1p-32;  // exact
            float p = (float)__dadd_rn((double)lo, mul_rounded(u, __dsub_rn((double)hi, (double)lo)));
            if (p >= hi) p = lo;
            int nl = 0, nr = 0;
            for (int base = 0; base < m; base += 64) {
                const int r = base + lane;
                const int row = r < m ? src[s0 + r] : 0;
                const float x = r < m ? X[(long)row * ldx + col] : 0.f;
                const bool left = r < m && x <= p, right = r < m && !left;
                const unsigned long long bl = __ballot(left), br = __ballot(right);
                const unsigned long long below = (1ull << lane) - 1ull;
                if (left) dst[s0 + nl + __popcll(bl & below)] = row;
                if (right) dst[s0 + m - 1 - nr - __popcll(br & below)] = row;
                nl += __popcll(bl);
                nr += __popcll(br);
            }
            if (lane == 0) {
                tree[node] = make_int2((int)col, __float_as_int(p));
                seg_start[2 * node] = (unsigned short)s0;
                seg_count[2 * node] = (unsigned short)nl;
                seg_start[2 * node + 1] = (unsigned short)(s0 + nl);
                seg_count[2 * node + 1] = (unsigned short)nr;
            }
        }
        __syncthreads();
    }
    int2* out = nodes + ((long)s * T + t) * N;
    for (int i = tid; i < N; i += kBlock) out[i] = tree[i];
}

template <int R>
__global__ __launch_bounds__(kBlock) void iforest_sums_kernel(const float* __restrict__ Xq, long ldq, int rows, int d,
                                                              const int2* __restrict__ nodes, int first, int T, int psi, int L,
                                                              const int64_t* __restrict__ cq, int64_t* __restrict__ sums, long ld_sums,
                                                              long block_stride) {
    __shared__ __attribute__((aligned(16))) int2 group[kIfGroupSlots];
    const int tid = threadIdx.x;
    const int N = 2 << L, per_group = kIfGroupSlots / N;
    const int z = blockIdx.y;
    const int2* trees = nodes + (long)(first + z) * T * N;
    Xq += (long)z * block_stride;
    const long r0 = (long)blockIdx.x * (R * kBlock) + tid;
    long row[R];
    int64_t total[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        row[r] = r0 + (long)r * kBlock;
        total[r] = 0;
    }
    for (int t0 = 0; t0 < T; t0 += per_group) {
        const int g = min(per_group, T - t0);
        __syncthreads();  // the previous group has been walked
        const int4* src = reinterpret_cast<const int4*>(trees + (long)t0 * N);  // N >= 4: a tree is a multiple of 16 bytes
        int4* dst = reinterpret_cast<int4*>(group);
        for (int i = tid; i < g * N / 2; i += kBlock) dst[i] = src[i];
        __syncthreads();
        for (int k = 0; k < g; ++k) {
            const int2* tree = group + k * N;
            int node[R];
#pragma unroll
            for (int r = 0; r < R; ++r) node[r] = 1;
            for (int e = 0; e < L; ++e) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int2 rec = tree[node[r]];
                    if (row[r] < rows && (unsigned)rec.x < (unsigned)d) {  // an internal node; a feature past d is never read
                        const float x = Xq[row[r] * ldq + rec.x];
                        node[r] = 2 * node[r] + (x <= __int_as_float(rec.y) ? 0 : 1);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int size = min(max(tree[node[r]].y, 0), psi);
                const int depth = 31 - __clz(node[r]);
                total[r] += ((int64_t)depth << 32) + cq[size];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (row[r] < rows) sums[(long)z * ld_sums + row[r]] = total[r];
}

__global__ __launch_bounds__(kBlock) void iforest_scores_kernel(const int64_t* __restrict__ sums, long ld_sums, int rows, double denom,
                                                                float* __restrict__ score, long ld_score) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    const long z = blockIdx.y;
    if (i < rows) score[z * ld_score + i] = (float)exp2(-((double)sums[z * ld_sums + i] / denom));
}

// ---- oblique cuts (SubspaceIForest(n_dims = q >= 2); the class docstring is the definition) ------------------------------
//   nodes    word 0 = the successful attempt (0 .. 3) of an internal node, -1 a leaf, -2 absent; word 1 as above.  The plane
//            of slot i is plane_col[i q .. i q + q) (columns of X, ascending, -1 in the unused places) and plane_w (0 there).
//   build    the skeleton above without its all-features scan: a node's wave draws an attempt's 21 Philox blocks one a lane,
//            chooses the m_s positions (lane k keeps the k-th smallest and its weight), projects the node's rows with lanes
//            over rows (m_s gathers a row, the same columns for all lanes) into LDS, reduces min and max and partitions from
//            the kept projections.  Loads: about psi m_s L per tree.
//   sums     the staging above for the 8-byte nodes; the planes (8 q bytes a slot, at most L of the N slots touched a row)
//            are read from global memory through L2.
constexpr int kIfMaxPlane = VGAN_IFOREST_MAX_PLANE;        // q
constexpr int kIfAttempts = 4;
constexpr unsigned kIfObliqueTag = 0x45494600u;            // "EIF\0": counter word 2 of every oblique draw

__device__ __forceinline__ float if_readlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(kBlock) void iforest_build_oblique_kernel(const float* __restrict__ X, unsigned long long n, int d,
                                                                       const int32_t* __restrict__ cand, const int32_t* __restrict__ cand_off,
                                                                       int first, int T, int psi, int L, int q, int w, unsigned long long seed,
                                                                       int2* __restrict__ nodes, int32_t* __restrict__ plane_col,
                                                                       float* __restrict__ plane_w) {
    __shared__ int rows[2][kIfMaxSamples];
    __shared__ int2 tree[kIfMaxSlots];
    __shared__ unsigned short seg_start[kIfMaxSlots], seg_count[kIfMaxSlots];
    __shared__ float proj[kIfMaxSamples];  // the projections of a level's rows, by their place in rows[]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = first + (int)(blockIdx.x / (unsigned)T), t = (int)(blockIdx.x % (unsigned)T);
    const unsigned long long id = (unsigned long long)s * (unsigned long long)T + (unsigned long long)t;
    const int N = 2 << L;
    const int off = cand_off[s], c = max(cand_off[s + 1] - off, 0), ms = min(q, c);
    const unsigned k0 = (unsigned)seed ^ (unsigned)id, k1 = (unsigned)(seed >> 32) ^ (unsigned)(id >> 32) ^ 0x5bd1e995u;
    const long slot0 = (long)id * N;

    for (int i = tid; i < psi; i += kBlock) rows[0][i] = (int)feistel_perm((unsigned long long)i, n, w, seed, id);
    for (int i = tid; i < N; i += kBlock) {
        tree[i] = make_int2(-2, 0);
        seg_start[i] = 0;
        seg_count[i] = (unsigned short)(i == 1 ? psi : kIfAbsent);
    }
    __syncthreads();

    for (int e = 0; e <= L; ++e) {
        const int* src = rows[e & 1];
        int* dst = rows[(e & 1) ^ 1];
        for (int node = (1 << e) + wave; node < (2 << e); node += kIfWaves) {
            const int m = seg_count[node];
            if (m == kIfAbsent) continue;  // the same for the whole wave
            const int s0 = seg_start[node];
            int a = kIfAttempts, pk = 0, colk = -1;  // lane k: the k-th smallest chosen position, its column and weight
            float wk = 0.f, lo = 0.f, hi = 0.f;
            unsigned w1 = 0u;
            if (m > 1 && e < L && ms > 0) {
                for (a = 0; a < kIfAttempts; ++a) {
                    // block `lane` of the attempt: 0 the threshold word, 1 .. 4 the positions, 5 + i weight i
                    unsigned ctr[4] = {(unsigned)node, (unsigned)(32 * a + lane), kIfObliqueTag, 0u};
                    philox4x32_10(ctr, k0, k1);
                    const unsigned long long sum4 = (unsigned long long)ctr[0] + ctr[1] + ctr[2] + ctr[3];
                    const float wl = (float)(((double)sum4 - 8589934590.0) * 0x1p-32);  // exact up to the one rounding
                    w1 = (unsigned)__builtin_amdgcn_readlane((int)ctr[1], 0);
                    pk = 0x7FFFFFFF;
                    wk = 0.f;
                    for (int i = 0; i < ms; ++i) {
                        const int i3 = i & 3;
                        const unsigned sel = i3 == 0 ? ctr[0] : i3 == 1 ? ctr[1] : i3 == 2 ? ctr[2] : ctr[3];
                        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)sel, 1 + (i >> 2));
                        int j = (int)(((unsigned long long)word * (unsigned long long)(c - i)) >> 32);
                        int r = 0;  // ascending walk: the places before r are <= j
                        for (; r < i; ++r) {
                            if (__builtin_amdgcn_readlane(pk, r) > j) break;
                            ++j;
                        }
                        const float wi = if_readlane(wl, 5 + i);
                        const int up = __shfl_up(pk, 1, 64);
                        const float upw = __shfl_up(wk, 1, 64);
                        if (lane > r && lane <= i) {
                            pk = up;
                            wk = upw;
                        }
                        if (lane == r) {
                            pk = j;
                            wk = wi;
                        }
                    }
                    // pk < c by construction; the clamp keeps a column of a malformed table inside the row
                    colk = lane < ms ? min(max(cand[off + pk], 0), d - 1) : -1;
                    lo = INFINITY;
                    hi = -INFINITY;
                    for (int base = 0; base < m; base += 64) {
                        const int r = base + lane;
                        const float* xr = X + (long)(r < m ? src[s0 + r] : src[s0]) * d;
                        double acc = 0.0;
                        for (int k = 0; k < ms; ++k) {  // ascending positions; every term rounded once, no fused multiply-add
                            const float x = if_value(xr[__builtin_amdgcn_readlane(colk, k)]);
                            acc = __dadd_rn(acc, mul_rounded_free((double)if_readlane(wk, k), (double)x));
                        }
                        const float zf = (float)acc;
                        if (r < m) {
                            proj[s0 + r] = zf;
                            lo = fminf(lo, zf);
                            hi = fmaxf(hi, zf);
                        }
                    }
                    lo = if_wave_min(lo);
                    hi = wave_max(hi);
                    if (!(lo == hi)) break;  // the same for the whole wave
                }
            }
            if (a == kIfAttempts) {
                if (lane == 0) tree[node] = make_int2(-1, m);
                continue;
            }
            // three separately rounded float64 operations (mul_rounded: the sum must not absorb the product)
            const double u = ((double)w1 + 0.5) * 0x1p-32;  // exact
            float p = (float)__dadd_rn((double)lo, mul_rounded(u, __dsub_rn((double)hi, (double)lo)));
            if (p >= hi) p = lo;
            int nl = 0, nr = 0;
            for (int base = 0; base < m; base += 64) {
                const int r = base + lane;
                const int row = r < m ? src[s0 + r] : 0;
                const float zf = r < m ? proj[s0 + r] : 0.f;  // written by this lane above
                const bool left = r < m && zf <= p, right = r < m && !left;
                const unsigned long long bl = __ballot(left), br = __ballot(right);
                const unsigned long long below = (1ull << lane) - 1ull;
                if (left) dst[s0 + nl + __popcll(bl & below)] = row;
                if (right) dst[s0 + m - 1 - nr - __popcll(br & below)] = row;
                nl += __popcll(bl);
                nr += __popcll(br);
            }
            if (lane < q) {
                plane_col[(slot0 + node) * q + lane] = colk;
                plane_w[(slot0 + node) * q + lane] = lane < ms ? wk : 0.f;
            }
            if (lane == 0) {
                tree[node] = make_int2(a, __float_as_int(p));
                seg_start[2 * node] = (unsigned short)s0;
                seg_count[2 * node] = (unsigned short)nl;
                seg_start[2 * node + 1] = (unsigned short)(s0 + nl);
                seg_count[2 * node + 1] = (unsigned short)nr;
            }
        }
        __syncthreads();
    }
    int2* out = nodes + slot0;
    for (int i = tid; i < N; i += kBlock) out[i] = tree[i];
    for (int i = tid; i < N * q; i += kBlock)  // the planes of the slots that are not internal: the others were stored above
        if (tree[i / q].x < 0) {
            plane_col[slot0 * q + i] = -1;
            plane_w[slot0 * q + i] = 0.f;
        }
}

template <int R>
__global__ __launch_bounds__(kBlock) void iforest_sums_oblique_kernel(const float* __restrict__ Xq, int rows, int d,
                                                                      const int2* __restrict__ nodes, const int32_t* __restrict__ plane_col,
                                                                      const float* __restrict__ plane_w, int first, int T, int psi, int L,
                                                                      int q, const int64_t* __restrict__ cq, int64_t* __restrict__ sums,
                                                                      long ld_sums) {
    __shared__ __attribute__((aligned(16))) int2 group[kIfGroupSlots];
    const int tid = threadIdx.x;
    const int N = 2 << L, per_group = kIfGroupSlots / N;
    const int z = blockIdx.y;
    const long tree0 = (long)(first + z) * T;
    const int2* trees = nodes + tree0 * N;
    const long r0 = (long)blockIdx.x * (R * kBlock) + tid;
    const float* xr[R];
    bool live[R];
    int64_t total[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        live[r] = r0 + (long)r * kBlock < rows;
        xr[r] = Xq + (live[r] ? r0 + (long)r * kBlock : 0L) * d;
        total[r] = 0;
    }
    for (int t0 = 0; t0 < T; t0 += per_group) {
        const int g = min(per_group, T - t0);
        __syncthreads();  // the previous group has been walked
        const int4* src = reinterpret_cast<const int4*>(trees + (long)t0 * N);  // N >= 4: a tree is a multiple of 16 bytes
        int4* dst = reinterpret_cast<int4*>(group);
        for (int i = tid; i < g * N / 2; i += kBlock) dst[i] = src[i];
        __syncthreads();
        for (int k = 0; k < g; ++k) {
            const int2* tree = group + k * N;
            const long slot0 = (tree0 + t0 + k) * N;
            int node[R];
#pragma unroll
            for (int r = 0; r < R; ++r) node[r] = 1;
            for (int e = 0; e < L; ++e) {
                bool inner[R], more[R];
                float thr[R];
                double acc[R];
                long at[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int2 rec = tree[node[r]];
                    inner[r] = more[r] = live[r] && (unsigned)rec.x < (unsigned)kIfAttempts;  // an internal node
                    thr[r] = __int_as_float(rec.y);
                    acc[r] = 0.0;
                    at[r] = (slot0 + node[r]) * q;
                }
                for (int f = 0; f < q; ++f) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (more[r]) {
                            const int col = plane_col[at[r] + f];
                            if ((unsigned)col >= (unsigned)d) {  // the plane ends at the first place that is no column of Xq
                                more[r] = false;
                            } else {
                                const float x = if_value(xr[r][col]);
                                acc[r] = __dadd_rn(acc[r], mul_rounded_free((double)plane_w[at[r] + f], (double)x));
                            }
                        }
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (inner[r]) node[r] = 2 * node[r] + ((float)acc[r] <= thr[r] ? 0 : 1);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int size = min(max(tree[node[r]].y, 0), psi);
                const int depth = 31 - __clz(node[r]);
                total[r] += ((int64_t)depth << 32) + cq[size];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (live[r]) sums[(long)z * ld_sums + r0 + (long)r * kBlock] = total[r];
}

}  // namespace vgan

using namespace vgan;

static bool iforest_shape_ok(int T, int psi, int L) {
    return T >= 1 && T <= VGAN_IFOREST_MAX_TREES && psi >= 2 && psi <= kIfMaxSamples && L >= 1 && (1 << L) >= psi && (1 << (L - 1)) < psi;
}

extern "C" int vgan_iforest_build(const float* X, int ldx, int64_t n, int d, const int32_t* feat, const int32_t* feat_off, int first,
                                  int count, int max_dims, int T, int psi, int L, uint64_t seed, int32_t* nodes, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && feat && feat_off && nodes && d > 0 && ldx >= d && n >= 2 && n <= 0x7FFFFFFFLL);
    VGAN_CHECK_ARG(first >= 0 && count > 0 && max_dims >= 1 && max_dims <= kIfMaxDims && max_dims <= d);
    VGAN_CHECK_ARG(iforest_shape_ok(T, psi, L) && psi <= n && (int64_t)count * T <= 0x7FFFFFFFLL);
    hipLaunchKernelGGL(iforest_build_kernel, dim3((unsigned)(count * T)), dim3(kBlock), 0, (hipStream_t)stream, X, (long)ldx,
                       (unsigned long long)n, feat, feat_off, first, T, psi, L, feistel_half_bits((unsigned long long)n),
                       (unsigned long long)seed, reinterpret_cast<int2*>(nodes), 0L, 0);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_iforest_build_blocks(const float* R, int64_t block_stride, int64_t n, int q, int first, int count, int T, int psi,
                                         int L, uint64_t seed, int32_t* nodes, vgan_stream_t stream) {
    VGAN_CHECK_ARG(R && nodes && q >= 1 && q <= kIfMaxDims && n >= 2 && n <= 0x7FFFFFFFLL && block_stride >= n * q);
    VGAN_CHECK_ARG(first >= 0 && count > 0 && iforest_shape_ok(T, psi, L) && psi <= n);
    VGAN_CHECK_ARG((int64_t)count * T <= 0x7FFFFFFFLL && ((int64_t)first + count) * T <= 0x7FFFFFFFLL);
    hipLaunchKernelGGL(iforest_build_kernel, dim3((unsigned)(count * T)), dim3(kBlock), 0, (hipStream_t)stream, R, (long)q,
                       (unsigned long long)n, (const int32_t*)nullptr, (const int32_t*)nullptr, first, T, psi, L,
                       feistel_half_bits((unsigned long long)n), (unsigned long long)seed, reinterpret_cast<int2*>(nodes),
                       (long)block_stride, q);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_iforest_path_sums(const float* Xq, int ldq, int rows, int d, const int32_t* nodes, int first, int count, int T,
                                      int psi, int L, const int64_t* cq, int64_t* sums, int64_t ld_sums, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && nodes && cq && sums && rows > 0 && d > 0 && ldq >= d && first >= 0 && count > 0 && count <= 65535);
    VGAN_CHECK_ARG(iforest_shape_ok(T, psi, L) && ld_sums >= rows);
    // four rows a thread once that still leaves two workgroups for every CU of the 256
    const long blocks4 = ((long)rows + 4 * kBlock - 1) / (4 * kBlock), blocks1 = ((long)rows + kBlock - 1) / kBlock;
    const hipStream_t st = (hipStream_t)stream;
    const int2* tn = reinterpret_cast<const int2*>(nodes);
    if (blocks4 * count >= 512)
        hipLaunchKernelGGL(iforest_sums_kernel<4>, dim3((unsigned)blocks4, count), dim3(kBlock), 0, st, Xq, (long)ldq, rows, d, tn, first, T,
                           psi, L, cq, sums, (long)ld_sums, 0L);
    else
        hipLaunchKernelGGL(iforest_sums_kernel<1>, dim3((unsigned)blocks1, count), dim3(kBlock), 0, st, Xq, (long)ldq, rows, d, tn, first, T,
                           psi, L, cq, sums, (long)ld_sums, 0L);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_iforest_path_sums_blocks(const float* Rq, int64_t block_stride, int rows, int q, const int32_t* nodes, int first,
                                             int count, int T, int psi, int L, const int64_t* cq, int64_t* sums, int64_t ld_sums,
                                             vgan_stream_t stream) {
    VGAN_CHECK_ARG(Rq && nodes && cq && sums && rows > 0 && q >= 1 && q <= kIfMaxDims && block_stride >= (int64_t)rows * q);
    VGAN_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && iforest_shape_ok(T, psi, L) && ld_sums >= rows);
    const long blocks4 = ((long)rows + 4 * kBlock - 1) / (4 * kBlock), blocks1 = ((long)rows + kBlock - 1) / kBlock;
    const hipStream_t st = (hipStream_t)stream;
    const int2* tn = reinterpret_cast<const int2*>(nodes);
    if (blocks4 * count >= 512)
        hipLaunchKernelGGL(iforest_sums_kernel<4>, dim3((unsigned)blocks4, count), dim3(kBlock), 0, st, Rq, (long)q, rows, q, tn, first, T,
                           psi, L, cq, sums, (long)ld_sums, (long)block_stride);
    else
        hipLaunchKernelGGL(iforest_sums_kernel<1>, dim3((unsigned)blocks1, count), dim3(kBlock), 0, st, Rq, (long)q, rows, q, tn, first, T,
                           psi, L, cq, sums, (long)ld_sums, (long)block_stride);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_iforest_scores(const int64_t* sums, int64_t ld_sums, int count, int rows, int64_t denom, float* score,
                                   int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(sums && score && count > 0 && count <= 65535 && rows > 0 && ld_sums >= rows && ld_score >= rows && denom > 0);
    hipLaunchKernelGGL(iforest_scores_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock), count), dim3(kBlock), 0, (hipStream_t)stream,
                       sums, (long)ld_sums, rows, (double)denom, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_iforest_build_oblique(const float* X, int64_t n, int d, const int32_t* cand, const int32_t* cand_off, int first,
                                          int count, int T, int psi, int L, int q, uint64_t seed, int32_t* nodes, int32_t* plane_col,
                                          float* plane_w, vgan_stream_t stream) {
    VGAN_CHECK_ARG(X && cand && cand_off && nodes && plane_col && plane_w && d > 0 && n >= 2 && n <= 0x7FFFFFFFLL);
    VGAN_CHECK_ARG(first >= 0 && count >= 1 && count <= 65535 && q >= 2 && q <= kIfMaxPlane);
    VGAN_CHECK_ARG(iforest_shape_ok(T, psi, L) && psi <= n && ((int64_t)first + count) * T <= 0x7FFFFFFFLL);
    hipLaunchKernelGGL(iforest_build_oblique_kernel, dim3((unsigned)(count * T)), dim3(kBlock), 0, (hipStream_t)stream, X,
                       (unsigned long long)n, d, cand, cand_off, first, T, psi, L, q, feistel_half_bits((unsigned long long)n),
                       (unsigned long long)seed, reinterpret_cast<int2*>(nodes), plane_col, plane_w);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_iforest_path_sums_oblique(const float* Xq, int rows, int d, const int32_t* nodes, const int32_t* plane_col,
                                              const float* plane_w, int first, int count, int T, int psi, int L, int q,
                                              const int64_t* cq, int64_t* sums, int64_t ld_sums, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && nodes && plane_col && plane_w && cq && sums && rows > 0 && d > 0 && first >= 0 && count >= 1 && count <= 65535);
    VGAN_CHECK_ARG(iforest_shape_ok(T, psi, L) && q >= 2 && q <= kIfMaxPlane && ld_sums >= rows);
    // the rule of vgan_iforest_path_sums: four rows a thread once that still leaves two workgroups for every CU
    const long blocks4 = ((long)rows + 4 * kBlock - 1) / (4 * kBlock), blocks1 = ((long)rows + kBlock - 1) / kBlock;
    const hipStream_t st = (hipStream_t)stream;
    const int2* tn = reinterpret_cast<const int2*>(nodes);
    if (blocks4 * count >= 512)
        hipLaunchKernelGGL(iforest_sums_oblique_kernel<4>, dim3((unsigned)blocks4, count), dim3(kBlock), 0, st, Xq, rows, d, tn, plane_col,
                           plane_w, first, T, psi, L, q, cq, sums, (long)ld_sums);
    else
        hipLaunchKernelGGL(iforest_sums_oblique_kernel<1>, dim3((unsigned)blocks1, count), dim3(kBlock), 0, st, Xq, rows, d, tn, plane_col,
                           plane_w, first, T, psi, L, q, cq, sums, (long)ld_sums);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

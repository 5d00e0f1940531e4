// The distance producer of the outlier kernels (outlier.hip: kNN, KDE; cluster.hip: k-means assignment): a workgroup owns
// 64 query rows of one subspace and walks the reference rows 64 at a time; the n_q x n_r distance matrix never exists.
// On top of it, the pairwise core of the kernel methods (KDE, OCSVM, SOS, KPCA): one kernel that stores an entry per pair
// (pair_matrix_kernel), one fixed-point row-sum sweep (fixed_point_row_sums), and the host side all launchers of the producer
// share (dist_args_ok, dist_grid, dispatch_engine).
#pragma once
#include <math.h>

#include <type_traits>

#include "gemm_core.hpp"

namespace vgan {

constexpr int kOTile = 64;  // query rows per workgroup = reference rows per tile
constexpr int kOFB = 32;    // features per LDS block of the exact engine
constexpr int kOLd = kOFB + 4;  // LDS row stride of those blocks (36 / 4 = 9 odd: conflict-free 16-byte reads)

__device__ __forceinline__ bool cand_less(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// An RBF kernel entry from an engine's d2 (outlier_ocsvm.hip, outlier_kpca.hip): float32 exp(-gamma d2), the argument formed
// in float64 and rounded once
__device__ __forceinline__ float rbf_entry(double gamma, float d2) { return expf((float)(-gamma * (double)d2)); }

// The RBF entry functors of pair_matrix_kernel: of(s) loads gamma_s once, and the result gives the entry of the pair (q, c);
// UNIT_DIAGONAL stores the pairs c == q as exactly 1 (a matrix of a block against itself)
template <bool UNIT_DIAGONAL>
struct RbfEntry {
    const double* __restrict__ gamma;
    struct Of {
        double g;
        __device__ __forceinline__ float operator()(int q, int c, float d2) const {
            return UNIT_DIAGONAL && c == q ? 1.f : rbf_entry(g, d2);
        }
    };
    __device__ __forceinline__ Of of(int s) const { return {gamma[s]}; }
};

// LDS of the distance producer's engine: the Gram tile's operand images and a 64 x 65 d2 tile, or the exact engine's
// two 64-row x 32-feature operand blocks
template <bool GRAM>
struct DistLds {
    using G = GemmTile<64, 64, 32, KC, KC, 4>;
    static constexpr int kFloats = GRAM ? G::kLdsFloats + kOTile * (kOTile + 1) : 2 * kOTile * kOLd;
};

// The distance producer shared by the knn, kde and k-means assignment kernels.  Grid (query blocks, J, chunk
// subspaces): the workgroup owns query rows [q0, q0 + 64) of chunk subspace blockIdx.z and slice blockIdx.y of its
// 64-row reference tiles.  For every tile at r0, lane l of wave w calls consume(d2, c0) with c0 = r0 + 16 w and
// d2[j] = d^2(q0 + l, c0 + j), j < 16; columns c0 + j >= nr (and rows q0 + l >= nq) hold values the consumer must
// skip.  A pair's d2 does not depend on the tile, slice or chunk that computes it.  lds: DistLds<GRAM>::kFloats floats,
// free again after the call.
template <bool GRAM, class Consume>
__device__ __forceinline__ void outlier_distances(const float* __restrict__ Pq, const float* __restrict__ sqq, int nq,
                                                  const float* __restrict__ Pr, const float* __restrict__ sqr, int nr,
                                                  const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                  int first, int splits, float* lds, Consume&& consume) {
    using G = typename DistLds<GRAM>::G;
    const int z = blockIdx.z, s = first + z, slice = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * kOTile;
    const int ds = feat_off[s + 1] - feat_off[s];
    const int w = (ds + 3) & ~3;
    const long base = col_off[s] - col_off[first];
    const float* Q = Pq + base * nq;
    const float* R = Pr + base * nr;
    if constexpr (GRAM) {  // norms of chunk subspace z: [count, n]
        sqq += (long)z * nq;
        sqr += (long)z * nr;
    }
    const int ntiles = (nr + kOTile - 1) / kOTile, per = (ntiles + splits - 1) / splits;
    const int t_begin = slice * per, t_end = min(ntiles, t_begin + per);

    if constexpr (GRAM) {
        float* dist = lds + G::kLdsFloats;  // [64][65]
        for (int t = t_begin; t < t_end; ++t) {
            const int r0 = t * kOTile;
            f32x16 acc[1][1];
            zero_acc(acc);
            G::template run<false>(Q, w, R, w, q0, r0, nq, nr, w, lds, nullptr, acc);
            const int col = G::sub_col(0);
            const float sc = r0 + col < nr ? sqr[r0 + col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = G::sub_row(0, r);
                const float sr = q0 + row < nq ? sqq[q0 + row] : 0.f;
                dist[row * (kOTile + 1) + col] = fmaxf(sr + sc - 2.f * acc[0][0][r], 0.f);
            }
            __syncthreads();
            float d2[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) d2[j] = dist[lane * (kOTile + 1) + 16 * wave + j];
            consume(d2, r0 + 16 * wave);
            __syncthreads();
        }
    } else {
        float* sQ = lds;  // [64][kOLd]
        float* sR = lds + kOTile * kOLd;
        // 64 rows x 32 features = 512 float4 per operand block: two per thread, zero outside [rows) x [w)
        auto stage = [&](float* dst, const float* src, int n, int row0, int f0) {
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int e = tid + kBlock * v, row = e >> 3, c = f0 + 4 * (e & 7);
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row0 + row < n && c < w) x = *reinterpret_cast<const float4*>(src + (long)(row0 + row) * w + c);
                *reinterpret_cast<float4*>(dst + row * kOLd + 4 * (e & 7)) = x;
            }
        };
        const bool q_resident = w <= kOFB;
        if (q_resident) stage(sQ, Q, nq, q0, 0);
        for (int t = t_begin; t < t_end; ++t) {
            const int r0 = t * kOTile;
            float d2[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) d2[j] = 0.f;
            for (int f0 = 0; f0 < w; f0 += kOFB) {
                __syncthreads();
                if (!q_resident) stage(sQ, Q, nq, q0, f0);
                stage(sR, R, nr, r0, f0);
                __syncthreads();
                const int nc = min(kOFB, w - f0) >> 2;
                for (int c = 0; c < nc; ++c) {
                    const float4 a = *reinterpret_cast<const float4*>(sQ + lane * kOLd + 4 * c);
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float4 b = *reinterpret_cast<const float4*>(sR + (16 * wave + j) * kOLd + 4 * c);
                        const float x = a.x - b.x, y = a.y - b.y, u = a.z - b.z, v = a.w - b.w;
                        d2[j] = fmaf(x, x, fmaf(y, y, fmaf(u, u, fmaf(v, v, d2[j]))));
                    }
                }
            }
            consume(d2, r0 + 16 * wave);
        }
    }
}

// out[z] = entry(q, c, d2(q, c)) for every pair of chunk subspace z, float32 [nq, nr] (BY_QUERY: lane l of a wave holds query
// row q0 + l and 16 neighbouring columns, a lane writes 64 consecutive bytes) or [nr, nq] (by reference row: the entry of the
// pair (q, c) goes to row c, so that the 64 lanes of a store write 64 consecutive floats).  entry.of(s) is taken once per
// workgroup, before the producer runs.
template <bool GRAM, bool BY_QUERY, class Entry>
__global__ __launch_bounds__(kBlock, 2) void pair_matrix_kernel(const float* __restrict__ Pq, const float* __restrict__ sqq, int nq,
                                                                const float* __restrict__ Pr, const float* __restrict__ sqr, int nr,
                                                                const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                                int first, int splits, Entry entry, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[DistLds<GRAM>::kFloats];
    const int z = blockIdx.z, lane = threadIdx.x & 63;
    const int q = blockIdx.x * kOTile + lane;
    const auto e = entry.of(first + z);
    float* o = out + (long)z * nq * nr;
    outlier_distances<GRAM>(Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, lds, [&](const float (&d2)[16], int c0) {
        if (q >= nq) return;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j;
            if (c < nr) o[BY_QUERY ? (long)q * nr + c : (long)c * nq + q] = e(q, c, d2[j]);
        }
    });
}

// acc[z nq + q] += the sum over the reference rows of this slice of tile(d2, c0), the unsigned 64-bit fixed-point contribution
// of the lane's 16 columns of a tile (0 from a lane whose row q0 + l >= nq has none).  The four waves of a row merge through
// LDS and wave 0, whose 64 lanes hold 64 consecutive rows, issues one atomicAdd per (slice, row): integer sums have no order,
// so acc is the same for every split.  lds: DistLds<GRAM>::kFloats floats.
template <bool GRAM, class Tile>
__device__ __forceinline__ void fixed_point_row_sums(const float* __restrict__ Pq, const float* __restrict__ sqq, int nq,
                                                     const float* __restrict__ Pr, const float* __restrict__ sqr, int nr,
                                                     const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                     int first, int splits, float* lds, unsigned long long* __restrict__ acc,
                                                     Tile&& tile) {
    static_assert(DistLds<GRAM>::kFloats >= 2 * kBlock, "merge scratch");
    const int z = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x * kOTile + lane;
    unsigned long long a = 0;
    outlier_distances<GRAM>(Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, lds,
                            [&](const float (&d2)[16], int c0) { a += tile(d2, c0); });
    __syncthreads();
    unsigned long long* la = reinterpret_cast<unsigned long long*>(lds);
    la[tid] = a;
    __syncthreads();
    if (wave == 0 && q < nq) atomicAdd(acc + (long)z * nq + q, la[lane] + la[kWave + lane] + la[2 * kWave + lane] + la[3 * kWave + lane]);
}

// ---- host side of every launch of the producer -------------------------------------------------------------------------------
// the engine is one of the two, the Gram engine has its norms, 1 <= splits <= 65535 (grid.y) and the operand blocks can be
// read 16 bytes at a time
inline bool dist_args_ok(int engine, bool norms, int splits, const void* Pq, const void* Pr) {
    return (engine == VGAN_OUTLIER_ENGINE_EXACT || (engine == VGAN_OUTLIER_ENGINE_GRAM && norms)) && splits >= 1 && splits <= 65535 &&
           aligned16(Pq) && aligned16(Pr);
}

inline dim3 dist_grid(int nq, int splits, int count) { return dim3((nq + kOTile - 1) / kOTile, splits, count); }

// launch(std::true_type) for the Gram engine, launch(std::false_type) for the exact one: launch(gram) names its kernel as
// kernel<decltype(gram)::value, ...>
template <class Launch>
inline void dispatch_engine(int engine, Launch&& launch) {
    if (engine == VGAN_OUTLIER_ENGINE_GRAM)
        launch(std::true_type{});
    else
        launch(std::false_type{});
}

template <bool BY_QUERY, class Entry>
inline void launch_pair_matrix(int engine, const float* Pq, const float* sqq, int nq, const float* Pr, const float* sqr, int nr,
                               const int32_t* feat_off, const int64_t* col_off, int first, int count, int splits, Entry entry,
                               float* out, hipStream_t st) {
    dispatch_engine(engine, [&](auto gram) {
        hipLaunchKernelGGL((pair_matrix_kernel<decltype(gram)::value, BY_QUERY, Entry>), dist_grid(nq, splits, count), dim3(kBlock), 0, st,
                           Pq, sqq, nq, Pr, sqr, nr, feat_off, col_off, first, splits, entry, out);
    });
}

}  // namespace vgan

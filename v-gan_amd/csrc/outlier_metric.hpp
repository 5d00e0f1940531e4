// The Minkowski-family distance producer of the outlier kernels (outlier.hip: vgan_outlier_knn_metric): Manhattan, Chebyshev
// and L_p over the uncentred packed blocks, on the vector ALU.  These norms do not factor as |q|^2 + |r|^2 - 2 q.r, so the
// matrix unit of the Gram engine is of no use; and the exact engine of outlier_dist.hpp (one query row by 16 reference rows
// per lane, 17 ds_read_b128 per 64 pair-features) is LDS-bound at the d_s of a few hundred this producer is for.
//
// Shape.  A workgroup owns 64 query rows and walks its slice of the 64-row reference tiles, as outlier_distances does.  The
// features of a tile pass through LDS 32 at a time ([64][36] images of both operands); thread (tx, ty) = (tid & 15, tid >> 4)
// keeps a 4 x 4 register tile, the pairs (query ty + 16 i, reference tx + 16 j): 8 ds_read_b128 per 64 pair-features, half of
// them broadcasts.  The 16 lanes of a ds_read_b128 group read 16 consecutive rows (row stride 36 floats: 16 distinct
// 4-bank windows) or at most two broadcast rows: no bank conflict.  A wave then spends 128 vector instructions (256 cycles of
// its SIMD) per 32 LDS cycles of the CU, so four waves keep the LDS array half busy and the vector ALU is the limit.  The next
// 32 features are loaded from global memory into registers while the present ones are summed.  The finished 64 x 64 tile
// goes through LDS ([64][65]) into the consumer layout of outlier_distances.
//
// The ranking value g of a pair (not the distance: every map g -> distance is monotone):
//   L1     sum_f |q_f - r_f|       float32, features ascending: subtract, add with |.| as an operand modifier: 2 operations
//                                  (inline assembly: see MetricL1)
//   Linf   max_f |q_f - r_f|       float32: subtract, max with |.|: at most 2 operations; exact apart from the one rounding of
//                                  q_f - r_f
//   Lp     sum_f |q_f - r_f|^p     float32, a term is exp2f(p log2f(|q_f - r_f|)) (0 for a zero difference: log2f(0) = -inf,
//                                  exp2f(-inf) = 0); no root.  A sum beyond FLT_MAX is +inf and such pairs compare equal.
// The zero padding of a packed row adds |0 - 0| = 0 to a sum and leaves a maximum of non-negative values alone.  The order of
// the operations of a pair is fixed by the feature index alone, so g does not depend on the tile, slice or chunk.  Equal rows
// give g = 0 exactly.
#pragma once
#include "outlier_dist.hpp"

namespace vgan {

// term(g, q, r): g after the feature with the values q and r
struct MetricL1 {
    // Spelt as the two instructions it is.  Left to the compiler the four features of a float4 are paired into v_pk_add_f32,
    // which has no |.| modifier: a packed subtract, two v_and and a packed add per two pair-features, each packed one at the
    // issue cost of two plain ones, plus the moves that line the pairs up: more than three operations a pair-feature.
    __device__ __forceinline__ float operator()(float g, float q, float r) const {
        float e, out;
        asm("v_sub_f32 %0, %1, %2" : "=v"(e) : "v"(q), "v"(r));
        asm("v_add_f32 %0, |%1|, %2" : "=v"(out) : "v"(e), "v"(g));
        return out;
    }
};
struct MetricLinf {  // compiles to a subtract per feature and one v_max3_f32 with |.| per two features
    __device__ __forceinline__ float operator()(float g, float q, float r) const { return fmaxf(g, fabsf(q - r)); }
};
struct MetricLp {
    float p;
    __device__ __forceinline__ float operator()(float g, float q, float r) const { return g + exp2f(p * log2f(fabsf(q - r))); }
};

// LDS of the producer: the two [64][36] operand images and the [64][65] tile of ranking values
constexpr int kMetricLdsFloats = 2 * kOTile * kOLd + kOTile * (kOTile + 1);

// Grid, ownership and consumer contract of outlier_distances: for every tile at r0 of the workgroup's slice, lane l of wave w
// calls consume(g, c0) with c0 = r0 + 16 w and g[j] = the ranking value of the pair (q0 + l, c0 + j), j < 16; columns c0 + j
// >= nr and rows q0 + l >= nq hold values the consumer must skip.  Pq / Pr: uncentred packed blocks.  lds: kMetricLdsFloats
// floats, free again after the call.
template <class Term, class Consume>
__device__ __forceinline__ void outlier_metric_distances(const float* __restrict__ Pq, int nq, const float* __restrict__ Pr, int nr,
                                                         const int32_t* __restrict__ feat_off, const int64_t* __restrict__ col_off,
                                                         int first, int splits, Term term, float* lds, Consume&& consume) {
    const int z = blockIdx.z, s = first + z, slice = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid & 15, ty = tid >> 4;
    const int q0 = blockIdx.x * kOTile;
    const int ds = feat_off[s + 1] - feat_off[s];
    const int w = (ds + 3) & ~3;
    const long base = col_off[s] - col_off[first];
    const float* Q = Pq + base * nq;
    const float* R = Pr + base * nr;
    const int ntiles = (nr + kOTile - 1) / kOTile, per = (ntiles + splits - 1) / splits;
    const int t_begin = slice * per, t_end = min(ntiles, t_begin + per);

    float* sQ = lds;  // [64][kOLd]
    float* sR = lds + kOTile * kOLd;
    float* tile = lds + 2 * kOTile * kOLd;  // [64][65]
    // 64 rows x 32 features = 512 float4 per operand block: two per thread, zero outside [rows) x [w)
    auto fetch = [&](float4 (&x)[2], const float* src, int n, int row0, int f0) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int e = tid + kBlock * v, row = e >> 3, c = f0 + 4 * (e & 7);
            x[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + row < n && c < w) x[v] = *reinterpret_cast<const float4*>(src + (long)(row0 + row) * w + c);
        }
    };
    auto put = [&](float* dst, const float4 (&x)[2]) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int e = tid + kBlock * v;
            *reinterpret_cast<float4*>(dst + (e >> 3) * kOLd + 4 * (e & 7)) = x[v];
        }
    };

    for (int t = t_begin; t < t_end; ++t) {
        const int r0 = t * kOTile;
        float g[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) g[i][j] = 0.f;
        float4 xq[2], xr[2];
        fetch(xq, Q, nq, q0, 0);
        fetch(xr, R, nr, r0, 0);
        for (int f0 = 0; f0 < w; f0 += kOFB) {
            __syncthreads();  // the images (and, at f0 = 0, the tile of the last round) are read no more
            put(sQ, xq);
            put(sR, xr);
            __syncthreads();
            if (f0 + kOFB < w) {  // the next block travels while this one is summed
                fetch(xq, Q, nq, q0, f0 + kOFB);
                fetch(xr, R, nr, r0, f0 + kOFB);
            }
            const int nc = min(kOFB, w - f0) >> 2;
            for (int c = 0; c < nc; ++c) {
                float4 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const float4*>(sQ + (ty + 16 * i) * kOLd + 4 * c);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(sR + (tx + 16 * j) * kOLd + 4 * c);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        g[i][j] = term(term(term(term(g[i][j], a[i].x, b[j].x), a[i].y, b[j].y), a[i].z, b[j].z), a[i].w, b[j].w);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[(ty + 16 * i) * (kOTile + 1) + tx + 16 * j] = g[i][j];
        __syncthreads();
        float out[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) out[j] = tile[lane * (kOTile + 1) + 16 * wave + j];
        consume(out, r0 + 16 * wave);
    }
}

}  // namespace vgan

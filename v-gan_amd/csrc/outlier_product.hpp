// The masked float64 product of the detectors whose per-feature terms do not depend on the subspace (ECOD, HBOS): every
// subspace is a 0/1-masked sum of a term matrix, one dense product with the mask [d, S] on v_mfma_f64_16x16x4_f64.
//
//   product  out^T [S, rows] = mask^T [S, d] x terms^T [d, rows]: A = the mask (row = subspace), B = the terms (column =
//            data row), so that the 16 lanes of a result row store 16 neighbouring data rows.  Workgroup tile 32 subspaces
//            x 64 rows, a wave 32 x 16 (two accumulators per plane, which covers the dependent latency of the
//            instruction), K staged through LDS 16 at a time and zero filled past d, S and rows.  Every output element
//            sees k = 0, 1, 2, ... in the same order whatever its position in a tile or a chunk.
#pragma once
#include "vgan_common.hpp"

namespace vgan {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kEcodBR = 64, kEcodBS = 32, kEcodKC = 16;  // product: rows, subspaces, K per staged tile

// M = 1: out = the masked sum of one term plane; M = 3: the elementwise max of the masked sums of three stacked planes
template <int M>
__global__ __launch_bounds__(kBlock) void ecod_product_kernel(const double* __restrict__ T, long rows, int d, const double* __restrict__ mask,
                                                              int ldm, int S, float* __restrict__ out, long ld_out) {
    __shared__ double lm[kEcodKC][kEcodBS + 1];     // mask tile [k][subspace]
    __shared__ double lt[M][kEcodKC][kEcodBR + 1];  // term tiles [k][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r0 = (long)blockIdx.x * kEcodBR;
    const int s0 = blockIdx.y * kEcodBS;
    f64x4 acc[M][2];
#pragma unroll
    for (int p = 0; p < M; ++p) acc[p][0] = acc[p][1] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int k0 = 0; k0 < d; k0 += kEcodKC) {
        __syncthreads();  // the previous tile has been read
        for (int e = tid; e < kEcodKC * kEcodBS; e += kBlock) {
            const int kk = e / kEcodBS, s = e % kEcodBS;
            lm[kk][s] = (k0 + kk < d && s0 + s < S) ? mask[(long)(k0 + kk) * ldm + s0 + s] : 0.0;
        }
#pragma unroll
        for (int p = 0; p < M; ++p)
            for (int e = tid; e < kEcodKC * kEcodBR; e += kBlock) {
                const int kk = e % kEcodKC, r = e / kEcodKC;
                lt[p][kk][r] = (k0 + kk < d && r0 + r < rows) ? T[((long)p * rows + r0 + r) * d + k0 + kk] : 0.0;
            }
        __syncthreads();
        const int steps = min(kEcodKC, (d - k0 + 3) & ~3);
        for (int ks = 0; ks < steps; ks += 4) {
            const int kk = ks + (lane >> 4);
            const double a0 = lm[kk][lane & 15], a1 = lm[kk][16 + (lane & 15)];
#pragma unroll
            for (int p = 0; p < M; ++p) {
                const double b = lt[p][kk][wave * 16 + (lane & 15)];
                acc[p][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[p][0], 0, 0, 0);
                acc[p][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[p][1], 0, 0, 0);
            }
        }
    }
    // f64 result layout: column = lane & 15 (the data row), row = (lane >> 4) + 4 i (the subspace)
    const long r = r0 + wave * 16 + (lane & 15);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int s = s0 + t * 16 + (lane >> 4) + 4 * i;
            double v = acc[0][t][i];
            if (M == 3) v = fmax(fmax(v, acc[1][t][i]), acc[2][t][i]);
            if (s < S && r < rows) out[(long)s * ld_out + r] = (float)v;
        }
}

}  // namespace vgan

// PCA outlier scores over the subspaces: the eigenpairs of the float64 covariance (or correlation) matrix of every subspace
// by a parallel cyclic Jacobi method, and score = sum_j w_j y_j^2 with y = V D^-1 (x - mu) as a full float64 product on the
// matrix unit.  The moments are vgan_maha_moments' (csrc/outlier_maha.hip).  Every sum and every rotation has a fixed order
// and there is no float atomic, so every published bit is the same from run to run.  The contract is the header's and the
// SubspacePCA docstring.
//
//   eigen    one workgroup per subspace.  scale_k = sqrt(C_kk) (0 -> 1) and M_ij = C_ij / (scale_i scale_j) when standardising,
//            else M = C; V starts as I.  A sweep is n - 1 rounds of a round-robin tournament on n = d_s rounded up to even
//            players: in round r position 0 holds player n - 1 and position k >= 1 player (k - 1 + r) mod (n - 1); pair i is
//            (a, b) = the players at positions i and n - 1 - i; a player >= d_s (the bye of an odd d_s) is a zero row that
//            nothing writes.  Step one of a round: a thread per pair reads m_aa, m_bb, m_ab and, unless |m_ab| <= 2^-53
//            sqrt(|m_aa m_bb|), takes zeta = (m_bb - m_aa) / (2 m_ab), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 /
//            sqrt(1 + t^2), s = c t.  Step two: the rotations of a round touch disjoint index pairs, so M <- J^T M J falls
//            into 2 x 2 blocks (pair I, pair J), each R_I^T (B R_J) on its own; a thread takes a block with I <= J and writes
//            it and its mirror image, so M stays symmetric to the bit; the block I = J becomes diag(m_aa - t m_ab, m_bb + t
//            m_ab) with exact zeros beside it.  The rows a, b of V (row j = the j-th component) turn likewise.  A block whose
//            two pairs were both skipped is not touched.  Two barriers a round.  A sweep that rotated nothing ends the
//            subspace (converged); max_sweeps bounds it.
//            d_s <= kPcaLds: M and V live in LDS (2 x 48 x 48 doubles = 36 KB); wider: M works in place in cov and V in the
//            output, through the one CU's cache, as maha_factor_kernel does.  In a round consecutive pairs hold consecutive
//            players (a ascending, b descending, modulo n - 1), so consecutive threads touch neighbouring elements.
//            Then lambda_j = m_jj; rank_j = #{k : lambda_k > lambda_j or (lambda_k == lambda_j and k < j)} (descending, ties by
//            the ascending diagonal position); a wave per component finds the entry of largest magnitude (lowest index on a
//            tie) and writes the row to its rank, negated if that entry is negative.
//   scores   outlier_moments.hpp's weighted projection (a workgroup per (subspace, 64 rows), 64 components a group, K in staged
//            slabs of 32 through LDS, a full K range) with z_k = (x_k - mu_k) inv_scale_k: a 16-row tile of V whose weights
//            are all 0 issues no MFMA, a group of 64 without weight is not staged.  A lane adds w_j y_j^2 over its components
//            in ascending order (j = (lane >> 4) + 4 i of each tile, tiles ascending), then the four lane groups are added as
//            (g + g^1) + (g^2 + g^3).  Which tiles are skipped depends on wt alone.
#include <math.h>

#include "outlier_moments.hpp"

namespace vgan {

constexpr int kPcaLds = VGAN_PCA_LDS_DIMS;               // the widest subspace whose M and V live in LDS
constexpr int kPcaMaxPairs = VGAN_MAHA_MAX_DIMS / 2;     // pairs of a round
constexpr double kPcaU = 1.1102230246251565e-16;         // 2^-53

__device__ __forceinline__ int pca_player(int pos, int r, int n) { return pos == 0 ? n - 1 : (pos - 1 + r) % (n - 1); }

// the sweeps on M [d, d] (row stride d) and Vt [d, d]; returns the sweeps run, *converged whether the last rotated nothing
__device__ int pca_sweeps(double* M, double* Vt, int d, int max_sweeps, double* pc, double* ps, double* pt, int* pa, int* pb,
                          unsigned char* prot, int* rotated, bool* converged) {
    const int tid = threadIdx.x;
    const int n = d + (d & 1), np = n / 2;
    const int half = (np + 1) / 2, wid = np + 1;
    int sweep = 0;
    *converged = false;
    while (sweep < max_sweeps) {
        if (tid == 0) *rotated = 0;
        __syncthreads();
        for (int r = 0; r < n - 1; ++r) {
            for (int i = tid; i < np; i += kBlock) {
                const int a = pca_player(i, r, n), b = pca_player(n - 1 - i, r, n);
                double c = 1.0, s = 0.0, t = 0.0;
                bool rot = false;
                if (a < d && b < d) {
                    const double app = M[(long)a * d + a], aqq = M[(long)b * d + b], apq = M[(long)a * d + b];
                    rot = fabs(apq) > kPcaU * sqrt(fabs(app * aqq));
                    if (rot) {
                        const double zeta = (aqq - app) / (2.0 * apq);
                        t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = c * t;
                        *rotated = 1;
                    }
                }
                pa[i] = a, pb[i] = b, pc[i] = c, ps[i] = s, pt[i] = t, prot[i] = rot ? 1 : 0;
            }
            __syncthreads();
            // the 2 x 2 blocks (I, J), I <= J: the triangle folded into half x (np + 1) items
            for (int e = tid; e < half * wid; e += kBlock) {
                const int fa = e / wid, fb = e - fa * wid;
                int I, J;
                if (fb < np - fa) {
                    I = fa, J = fa + fb;
                } else {
                    I = np - 1 - fa, J = I + fb - (np - fa);
                    if (I == fa) continue;  // the middle row of an odd np is taken once
                }
                if (!(prot[I] | prot[J])) continue;
                const int p1 = pa[I], q1 = pb[I];
                if (I == J) {
                    const double app = M[(long)p1 * d + p1], aqq = M[(long)q1 * d + q1], apq = M[(long)p1 * d + q1], t = pt[I];
                    M[(long)p1 * d + p1] = app - t * apq;
                    M[(long)q1 * d + q1] = aqq + t * apq;
                    M[(long)p1 * d + q1] = 0.0;
                    M[(long)q1 * d + p1] = 0.0;
                    continue;
                }
                const int p2 = pa[J], q2 = pb[J];
                const bool vp1 = p1 < d, vq1 = q1 < d, vp2 = p2 < d, vq2 = q2 < d;
                const double c1 = pc[I], s1 = ps[I], c2 = pc[J], s2 = ps[J];
                const double x11 = (vp1 && vp2) ? M[(long)p1 * d + p2] : 0.0, x12 = (vp1 && vq2) ? M[(long)p1 * d + q2] : 0.0;
                const double x21 = (vq1 && vp2) ? M[(long)q1 * d + p2] : 0.0, x22 = (vq1 && vq2) ? M[(long)q1 * d + q2] : 0.0;
                const double y11 = c2 * x11 - s2 * x12, y12 = s2 * x11 + c2 * x12;
                const double y21 = c2 * x21 - s2 * x22, y22 = s2 * x21 + c2 * x22;
                const double z11 = c1 * y11 - s1 * y21, z12 = c1 * y12 - s1 * y22;
                const double z21 = s1 * y11 + c1 * y21, z22 = s1 * y12 + c1 * y22;
                if (vp1 && vp2) M[(long)p1 * d + p2] = z11, M[(long)p2 * d + p1] = z11;
                if (vp1 && vq2) M[(long)p1 * d + q2] = z12, M[(long)q2 * d + p1] = z12;
                if (vq1 && vp2) M[(long)q1 * d + p2] = z21, M[(long)p2 * d + q1] = z21;
                if (vq1 && vq2) M[(long)q1 * d + q2] = z22, M[(long)q2 * d + q1] = z22;
            }
            for (int e = tid; e < np * d; e += kBlock) {
                const int i = e / d, k = e - i * d;
                if (!prot[i]) continue;
                double* ra = Vt + (long)pa[i] * d + k;
                double* rb = Vt + (long)pb[i] * d + k;
                const double va = *ra, vb = *rb, c = pc[i], s = ps[i];
                *ra = c * va - s * vb;
                *rb = s * va + c * vb;
            }
            __syncthreads();
        }
        ++sweep;
        const int any = *rotated;
        __syncthreads();
        if (!any) {
            *converged = true;
            break;
        }
    }
    return sweep;
}

// status: bit 0 tr M == 0, bit 1 not converged within max_sweeps
__global__ __launch_bounds__(kBlock) void pca_eigen_kernel(double* cov, const int64_t* __restrict__ sq_off,
                                                           const int32_t* __restrict__ feat_off, int first, int standardize,
                                                           int max_sweeps, double* __restrict__ scale_out, double* __restrict__ evals,
                                                           double* Vall, int32_t* __restrict__ sweeps_out, int32_t* __restrict__ status) {
    __shared__ double lm[kPcaLds * kPcaLds], lv[kPcaLds * kPcaLds];
    __shared__ double prm[3 * kPcaMaxPairs];  // c, s, t of the pairs of a round; afterwards the d eigenvalues
    __shared__ int pidx[2 * kPcaMaxPairs];    // a, b of the pairs of a round; afterwards the d ranks
    __shared__ unsigned char prot[kPcaMaxPairs];
    __shared__ double red[kBlock / kWave];
    __shared__ int rotated;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = first + blockIdx.x;
    const int f0 = feat_off[s], d = feat_off[s + 1] - f0;
    const long dd = (long)d * d;
    double* C = cov + sq_off[s];
    double* Vout = Vall + sq_off[s];
    const bool lds = d <= kPcaLds;
    double* M = lds ? lm : C;
    double* Vt = lds ? lv : Vout;

    for (int i = tid; i < d; i += kBlock) {
        const double sc = standardize ? sqrt(C[(long)i * d + i]) : 1.0;
        scale_out[f0 + i] = sc == 0.0 ? 1.0 : sc;
    }
    __syncthreads();
    for (long e = tid; e < dd; e += kBlock) {
        const int i = (int)(e / d), j = (int)(e % d);
        const double c = C[e];
        M[e] = standardize ? c / (scale_out[f0 + i] * scale_out[f0 + j]) : c;
        Vt[e] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    double tr = 0.0;
    for (int i = tid; i < d; i += kBlock) tr += M[(long)i * d + i];
    tr = wave_sum(tr);
    if (lane == 0) red[wave] = tr;
    __syncthreads();
    tr = ((red[0] + red[1]) + red[2]) + red[3];

    bool converged;
    const int sweeps = pca_sweeps(M, Vt, d, max_sweeps, prm, prm + kPcaMaxPairs, prm + 2 * kPcaMaxPairs, pidx, pidx + kPcaMaxPairs,
                                  prot, &rotated, &converged);
    if (tid == 0) {
        sweeps_out[s] = sweeps;
        status[s] = (tr == 0.0 ? 1 : 0) | (converged ? 0 : 2);
    }
    // the order: descending, ties by the ascending diagonal position
    double* lam = prm;
    for (int j = tid; j < d; j += kBlock) lam[j] = M[(long)j * d + j];
    __syncthreads();
    for (int j = tid; j < d; j += kBlock) {
        const double lj = lam[j];
        int rank = 0;
        for (int k = 0; k < d; ++k) {
            const double lk = lam[k];
            rank += (lk > lj || (lk == lj && k < j)) ? 1 : 0;
        }
        pidx[j] = rank;
        evals[f0 + rank] = lj;
    }
    __syncthreads();
    // the sign, and the rows to their ranks: from LDS straight to the output, otherwise through cov (M is no longer needed)
    double* dst = lds ? Vout : C;
    for (int j = wave; j < d; j += kBlock / kWave) {
        const double* row = Vt + (long)j * d;
        double best = -1.0, val = 0.0;
        int at = d;
        for (int k = lane; k < d; k += kWave) {
            const double v = row[k], m = fabs(v);
            if (m > best) best = m, val = v, at = k;  // k ascends: the first of equal magnitudes stays
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64), ov = __shfl_xor(val, o, 64);
            const int oa = __shfl_xor(at, o, 64);
            if (ob > best || (ob == best && oa < at)) best = ob, val = ov, at = oa;
        }
        const double sign = val < 0.0 ? -1.0 : 1.0;
        double* out = dst + (long)pidx[j] * d;
        for (int k = lane; k < d; k += kWave) out[k] = sign * row[k];
    }
    if (!lds) {
        __syncthreads();
        for (long e = tid; e < dd; e += kBlock) Vout[e] = C[e];
    }
}

__global__ __launch_bounds__(kBlock) void pca_scores_kernel(const float* __restrict__ Xq, long ldq, int rows, const int32_t* __restrict__ feat,
                                                            const int32_t* __restrict__ feat_off, const int64_t* __restrict__ sq_off,
                                                            int first, const double* __restrict__ mean, const double* __restrict__ inv_scale,
                                                            const double* __restrict__ Vall, const double* __restrict__ wt,
                                                            float* __restrict__ score, long ld_score) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = first + blockIdx.y;
    const int f0 = feat_off[s], d = feat_off[s + 1] - f0;
    const long r0 = (long)blockIdx.x * kMomBR;
    const double total = weighted_projection_sqnorm(rows, r0, d, Vall + sq_off[s], wt + f0, [&](long row, int k) {
        return ((double)Xq[row * ldq + feat[f0 + k]] - mean[f0 + k]) * inv_scale[f0 + k];
    });
    const long row = r0 + wave * kMomT + (lane & 15);
    if (lane < 16 && row < rows) score[(long)s * ld_score + row] = (float)total;
}

}  // namespace vgan

using namespace vgan;

static bool pca_range_ok(int first, int count) { return first >= 0 && count > 0 && count <= 65535; }

extern "C" int vgan_pca_eigen(double* cov, const int64_t* sq_off, const int32_t* feat_off, int first, int count, int max_dims,
                              int standardize, int max_sweeps, double* scale, double* evals, double* V, int32_t* sweeps,
                              int32_t* status, vgan_stream_t stream) {
    VGAN_CHECK_ARG(cov && sq_off && feat_off && scale && evals && V && sweeps && status && pca_range_ok(first, count));
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= VGAN_MAHA_MAX_DIMS && max_sweeps >= 1 && (standardize == 0 || standardize == 1));
    hipLaunchKernelGGL(pca_eigen_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, cov, sq_off, feat_off, first, standardize,
                       max_sweeps, scale, evals, V, sweeps, status);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_pca_scores(const float* Xq, int ldq, int rows, int d, const int32_t* feat, const int32_t* feat_off,
                               const int64_t* sq_off, int first, int count, int max_dims, const double* mean, const double* inv_scale,
                               const double* V, const double* wt, float* score, int64_t ld_score, vgan_stream_t stream) {
    VGAN_CHECK_ARG(Xq && feat && feat_off && sq_off && mean && inv_scale && V && wt && score && pca_range_ok(first, count));
    VGAN_CHECK_ARG(d > 0 && ldq >= d && rows > 0 && rows <= VGAN_MAHA_MAX_ROWS && ld_score >= rows);
    VGAN_CHECK_ARG(max_dims >= 1 && max_dims <= VGAN_MAHA_MAX_DIMS);
    const dim3 grid((rows + kMomBR - 1) / kMomBR, count);
    hipLaunchKernelGGL(pca_scores_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, Xq, (long)ldq, rows, feat, feat_off, sq_off, first, mean,
                       inv_scale, V, wt, score, (long)ld_score);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

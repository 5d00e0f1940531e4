// Layer routines of the small MLPs that one workgroup owns for a whole launch: the autoencoders (outlier_ae.hip, a bias in
// every layer) and the Deep SVDD encoders (outlier_svdd.hip, no bias anywhere).  BIAS is a compile-time switch; its `true`
// instantiation is the autoencoder's code as it was before the routines moved here.
//   image      a layer is K-MAJOR [K][N] (W[o, i] at i N + o); with BIAS row K of the same image is the bias (its input is the
//              constant 1), so the forward reads it and the update walks it without a second rule.
//   values     every product is ONE chain of fmaf in ascending order of the summation index, starting from 0: over k for a
//              unit (then the bias, if any, is added), over the output units f for an error passed down, over the batch rows i
//              for a gradient.  A chain belongs to one thread, so no value depends on the launch, the chunk or the address
//              space of the activations (P: LDS or a private slice of a scratch buffer in global memory).
#pragma once

#include "vgan_common.hpp"

namespace vgan {

constexpr int kAeBlock = 1024;  // 16 waves on the one CU a net owns: the weight reads of a step are latency, not bandwidth
constexpr int kAeRows = VGAN_AE_ROW_TILE;
constexpr int kAeUnroll = 8;  // weight loads a thread keeps in flight in a product chain

typedef __attribute__((address_space(3))) float ae_lds_f;

struct AeAdam {
    float b1, omb1, b2, omb2, eps, wd;
    double lr;
};

__host__ __device__ inline int ae_pitch(int w) { return w | 1; }  // odd: the rows of a column lie in different banks

__device__ __forceinline__ float ae_activate(float a, int act) {
    return act == VGAN_AE_ACT_RELU ? fmaxf(a, 0.f) : (float)tanh((double)a);
}

// z[i][f] = float32((double(x) - mean) / scale) of the rows rowidx[0 .. rows) and the features of the subspace
template <class P>
__device__ __forceinline__ void ae_stage(const float* __restrict__ X, long ldx, const int* rowidx, int rows, const int32_t* __restrict__ feat,
                                         const double* __restrict__ mean, const double* __restrict__ scale, int ds, P z, int pz) {
    for (int idx = threadIdx.x; idx < rows * ds; idx += kAeBlock) {
        const int i = idx / ds, f = idx - i * ds;
        const long col = feat[f];
        z[i * pz + f] = (float)(((double)X[(long)rowidx[i] * ldx + col] - mean[col]) / scale[col]);
    }
}

// epi(i, o, bias_o + sum_k in[i][k] W[o, k]) for every row i < rows and unit o < N (without BIAS the sum alone): the lanes
// of a wave take neighbouring units and a thread four rows, which share every weight it loads; row K of the image is the bias
template <bool BIAS, class P, class Epi>
__device__ __forceinline__ void ae_forward(P in, int pin, int K, const float* Wt, int N, int rows, Epi epi) {
    const int groups = (rows + 3) >> 2;
    for (int item = threadIdx.x; item < groups * N; item += kAeBlock) {
        const int g = item / N, o = item - g * N, i0 = g << 2;
        P r0 = in + min(i0, rows - 1) * pin, r1 = in + min(i0 + 1, rows - 1) * pin;
        P r2 = in + min(i0 + 2, rows - 1) * pin, r3 = in + min(i0 + 3, rows - 1) * pin;
        const float* w = Wt + o;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int k = 0;
        for (; k + kAeUnroll <= K; k += kAeUnroll) {  // the weights of kAeUnroll steps are in flight together; the chain stays k ascending
            float wk[kAeUnroll];
#pragma unroll
            for (int u = 0; u < kAeUnroll; ++u) wk[u] = w[(long)(k + u) * N];
#pragma unroll
            for (int u = 0; u < kAeUnroll; ++u) {
                a0 = fmaf(r0[k + u], wk[u], a0);
                a1 = fmaf(r1[k + u], wk[u], a1);
                a2 = fmaf(r2[k + u], wk[u], a2);
                a3 = fmaf(r3[k + u], wk[u], a3);
            }
        }
        for (; k < K; ++k) {
            const float wk = w[(long)k * N];
            a0 = fmaf(r0[k], wk, a0);
            a1 = fmaf(r1[k], wk, a1);
            a2 = fmaf(r2[k], wk, a2);
            a3 = fmaf(r3[k], wk, a3);
        }
        if constexpr (BIAS) {
            const float b = w[(long)K * N];
            a0 += b, a1 += b, a2 += b, a3 += b;
        }
        epi(i0, o, a0);
        if (i0 + 1 < rows) epi(i0 + 1, o, a1);
        if (i0 + 2 < rows) epi(i0 + 2, o, a2);
        if (i0 + 3 < rows) epi(i0 + 3, o, a3);
    }
}

// down[i][k] = sum_f delta[i][f] W[f, k], f ascending: the lanes of a wave take neighbouring rows (odd pitches: no bank
// conflict) and read the same weights, a thread four inputs k
template <class P>
__device__ __forceinline__ void ae_backprop(P delta, int pd, int N, const float* Wt, int K, int rows, P down, int pt) {
    const int kgs = (K + 3) >> 2;
    for (int item = threadIdx.x; item < kgs * rows; item += kAeBlock) {
        const int g = item / rows, i = item - g * rows, k0 = g << 2;
        const float* w0 = Wt + (long)min(k0, K - 1) * N;
        const float* w1 = Wt + (long)min(k0 + 1, K - 1) * N;
        const float* w2 = Wt + (long)min(k0 + 2, K - 1) * N;
        const float* w3 = Wt + (long)min(k0 + 3, K - 1) * N;
        P dr = delta + i * pd;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int f = 0;
        for (; f + kAeUnroll / 2 <= N; f += kAeUnroll / 2) {
            float v0[kAeUnroll / 2], v1[kAeUnroll / 2], v2[kAeUnroll / 2], v3[kAeUnroll / 2];
#pragma unroll
            for (int u = 0; u < kAeUnroll / 2; ++u) v0[u] = w0[f + u], v1[u] = w1[f + u], v2[u] = w2[f + u], v3[u] = w3[f + u];
#pragma unroll
            for (int u = 0; u < kAeUnroll / 2; ++u) {
                const float d = dr[f + u];
                a0 = fmaf(d, v0[u], a0);
                a1 = fmaf(d, v1[u], a1);
                a2 = fmaf(d, v2[u], a2);
                a3 = fmaf(d, v3[u], a3);
            }
        }
        for (; f < N; ++f) {
            const float d = dr[f];
            a0 = fmaf(d, w0[f], a0);
            a1 = fmaf(d, w1[f], a1);
            a2 = fmaf(d, w2[f], a2);
            a3 = fmaf(d, w3[f], a3);
        }
        P out = down + i * pt + k0;
        out[0] = a0;
        if (k0 + 1 < K) out[1] = a1;
        if (k0 + 2 < K) out[2] = a2;
        if (k0 + 3 < K) out[3] = a3;
    }
}

// Adam of one parameter from its gradient sum g and the values th, m, v it holds (the element-wise sequence of
// SubspaceAutoEncoder's docstring)
__device__ __forceinline__ void ae_adam(float& th, float& m, float& v, float g, const AeAdam& h, float lrc, float sc2) {
    g = fmaf(h.wd, th, g);
    m = fmaf(h.b1, m, h.omb1 * g);
    v = fmaf(h.b2, v, (h.omb2 * g) * g);
    const float den = sqrtf(v) / sc2 + h.eps;
    th = th - (lrc * m) / den;
}

// g[o, k] = sum_i delta[i][o] in[i][k], i ascending, and Adam behind it, in place; with BIAS k runs to K with in[i][K] = 1
// (the bias), else to K - 1.  The lanes of a wave take neighbouring units o (contiguous parameters), a thread four inputs k.
template <bool BIAS, class P>
__device__ __forceinline__ void ae_update(P delta, int pd, int N, P in, int pa, int K, int rows, float* theta, long P_n, const AeAdam& h,
                                          float lrc, float sc2) {
    const int Kp = BIAS ? K + 1 : K;  // rows of the image
    const int kgs = (Kp + 3) >> 2;
    for (int item = threadIdx.x; item < kgs * N; item += kAeBlock) {
        const int q = item / N, o = item - q * N, k0 = q << 2;
        const int c0 = min(k0, K - 1), c1 = min(k0 + 1, K - 1), c2 = min(k0 + 2, K - 1), c3 = min(k0 + 3, K - 1);
        const bool one0 = BIAS && k0 >= K, one1 = BIAS && k0 + 1 >= K, one2 = BIAS && k0 + 2 >= K, one3 = BIAS && k0 + 3 >= K;
        // the four parameters (k0 + j) N + o; those past the last row repeat the first and are not stored.  Their twelve loads
        // are in flight under the gradient chains
        long e[4];
        float th[4], m[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = (long)(k0 + j < Kp ? k0 + j : k0) * N + o;
            th[j] = theta[e[j]], m[j] = theta[P_n + e[j]], v[j] = theta[2 * P_n + e[j]];
        }
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
        for (int i = 0; i < rows; ++i) {
            const float d = delta[i * pd + o];
            P ar = in + i * pa;
            g0 = fmaf(d, one0 ? 1.f : ar[c0], g0);
            g1 = fmaf(d, one1 ? 1.f : ar[c1], g1);
            g2 = fmaf(d, one2 ? 1.f : ar[c2], g2);
            g3 = fmaf(d, one3 ? 1.f : ar[c3], g3);
        }
        const float g[4] = {g0, g1, g2, g3};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ae_adam(th[j], m[j], v[j], g[j], h, lrc, sc2);
            if (k0 + j < Kp) theta[e[j]] = th[j], theta[P_n + e[j]] = m[j], theta[2 * P_n + e[j]] = v[j];
        }
    }
}

// D[i][k] = down[i][k] act'(h[i][k]) in place of the activations h of the layer below
template <class P>
__device__ __forceinline__ void ae_derivative(P in, int pin, P down, int pt, int K, int rows, int act) {
    const bool relu = act == VGAN_AE_ACT_RELU;
    for (int idx = threadIdx.x; idx < rows * K; idx += kAeBlock) {
        const int i = idx / K, k = idx - i * K;
        const float h = in[i * pin + k];
        in[i * pin + k] = down[i * pt + k] * (relu ? (h > 0.f ? 1.f : 0.f) : fmaf(-h, h, 1.f));
    }
}

// lets a kernel take VGAN_AE_LDS_FLOATS of dynamic LDS
template <class Kernel>
static int ae_allow_lds(Kernel kernel, const char* file, int line) {
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                VGAN_AE_LDS_FLOATS * (int)sizeof(float));
    if (attr != hipSuccess) {
        set_error("%s:%d: hipFuncSetAttribute failed: %s", file, line, hipGetErrorString(attr));
        return VGAN_ERR_HIP;
    }
    return VGAN_OK;
}

}  // namespace vgan

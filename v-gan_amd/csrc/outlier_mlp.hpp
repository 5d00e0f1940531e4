// The core of the trained-MLP detectors: the small nets that one workgroup owns for a whole launch.  An OBJECTIVE (a struct of
// compile-time traits and a few inlined hooks) is all a detector adds: AeObjective in outlier_ae.hip (mirrored layers, a bias in
// every layer, the target is the input) and SvddObjective in outlier_svdd.hip (h_1 .. h_L, no bias, the target is a centre).
// Block b = the subspace at position b; its net has the layers K_0 = d_s -> N_0 -> .. -> N_{nl-1} of mlp_outputs, the activation
// after every layer but the last.
//
//   state      of a block: theta, m, v, P floats each (P = sum_l (K_l + bias) N_l), one after the other.  Inside each, layer after
//              layer, W_l K-MAJOR as [K_l][N_l] (W_l[o, i] at i N_l + o); with a bias, b_l [N_l] follows as row K_l of the same
//              image (its input is the constant 1), so the forward reads it and the update walks it without a second rule.  The
//              64 lanes of a wave that compute 64 neighbouring outputs read 256 contiguous bytes of every k.
//   init       W_l[o, i] (and b_l[o]) from the Philox4x32-10 words of counter (e >> 2, 0, tag + l, 0), e = o K_l + i, the biases
//              at e = N_l K_l + o, key (lo32(seed) ^ lo32(b), hi32(seed) ^ hi32(b) ^ 0x5bd1e995): word e & 3 is w, u = (w + 0.5)
//              2^-32 in float64, value float32((2 u - 1) c_l), c_l = 1 / sqrt(K_l) from the host.  m = v = 0.
//   train      ONE WORKGROUP OWNS ONE NET FOR THE WHOLE LAUNCH and runs step after step: the batch rows (feistel_perm) are
//              gathered from X through the feature list and standardised while staged; the forward keeps every activation of
//              the batch; the last layer leaves r = out - target; the loss sum r^2 / cells and the output error r float32(2 /
//              cells), cells from the objective; then layer by layer from the last: the error of the layer below through the
//              weights as they still are, the weight-gradient products with Adam behind each element (the gradient is a
//              register), the derivative of the activation.  Workgroups never wait for each other.  The activations live in
//              LDS while mlp_act_floats of the batch fit VGAN_AE_LDS_FLOATS, else in a slice of a scratch buffer in global
//              memory that only its own workgroup touches (it stays in L2): the same code through the other address space,
//              the same bits.  Where each activation sits in that space is the objective's (place).
//   scores     one workgroup per (block, tile of VGAN_AE_ROW_TILE = 32 rows) runs the forward through the same layer routine;
//              the objective runs the last layer and finishes the tile (a score per row, the raw output, column sums).
//   values     every product is ONE chain of fmaf in ascending order of the summation index, starting from 0: over k for a
//              unit (then the bias, if any, is added), over the output units f for an error passed down, over the batch rows i
//              for a gradient.  A chain belongs to one thread, so no value depends on the launch, the chunk, the address space
//              of the activations (P: LDS or a private slice of the scratch buffer) or which other blocks share the launch.
#pragma once

#include <type_traits>

#include "optim_common.hpp"
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

// ---- errors -------------------------------------------------------------------------------------------------------------
// The shared host routines report an error at the entry that called them: its file and line (MLP_HERE) with the failed condition
struct MlpSite {
    const char* file;
    int line;
};
#define MLP_HERE (::vgan::MlpSite{__FILE__, __LINE__})

// ---- the net ------------------------------------------------------------------------------------------------------------
// An objective O supplies: kBias, kMirrored, kCenter (a centre [count][w] is the target), kMaxLayers (the most layers of its
// shape: the size of the per-layer register arrays), loss_cells, center_lds, place, target, last_layer, finish.
constexpr int kMlpMaxLayers = 2 * VGAN_AE_MAX_HIDDEN;

struct MlpNet {
    int nl;                    // layers: 2 L mirrored, else L
    int width[kMlpMaxLayers];  // outputs of layer l; 0 for the last layer of a mirrored net, which has d_s
    int act;                   // VGAN_AE_ACT_*
    int wmax;                  // the widest of the given widths
};

template <class O>
__host__ __device__ inline int mlp_outputs(const MlpNet& net, int l, int ds) {
    return O::kMirrored && l == net.nl - 1 ? ds : net.width[l];
}
template <class O>
__host__ __device__ inline long mlp_params(const MlpNet& net, int ds) {
    long p = 0;
    int K = ds;
    for (int l = 0; l < net.nl; ++l) {
        const int N = mlp_outputs<O>(net, l, ds);
        p += (long)(K + (O::kBias ? 1 : 0)) * N;
        K = N;
    }
    return p;
}
// floats of the activations of `rows` rows: z, the output of every layer (a mirrored net's last: only when training, as the
// output error; when scoring it goes where the objective puts it) and, when training, one passed-down error
template <class O>
inline long mlp_act_floats(const MlpNet& net, int ds, int rows, bool train) {
    long f = (long)ae_pitch(ds) + (train ? ae_pitch(net.wmax) : 0);
    for (int l = 0; l < net.nl; ++l)
        if (l + 1 < net.nl || !O::kMirrored) f += ae_pitch(net.width[l]);
        else if (train) f += ae_pitch(ds);
    return f * rows;
}

// the net of the arguments; false when a size is out of range
inline bool mlp_net(int n_hidden, const int32_t* hidden, int activation, bool mirrored, MlpNet* net) {
    if (n_hidden < 1 || n_hidden > VGAN_AE_MAX_HIDDEN || !hidden) return false;
    if (activation != VGAN_AE_ACT_TANH && activation != VGAN_AE_ACT_RELU) return false;
    net->nl = mirrored ? 2 * n_hidden : n_hidden;
    net->wmax = 0;
    for (int l = 0; l < kMlpMaxLayers; ++l) net->width[l] = 0;
    for (int l = 0; l < n_hidden; ++l) {
        if (hidden[l] < 1 || hidden[l] > VGAN_AE_MAX_WIDTH) return false;
        net->width[l] = hidden[l];
        if (mirrored) net->width[2 * n_hidden - 2 - l] = hidden[l];
        if (hidden[l] > net->wmax) net->wmax = hidden[l];
    }
    net->act = activation;
    return true;
}

// ---- init ---------------------------------------------------------------------------------------------------------------
template <class O>
__global__ __launch_bounds__(kBlock) void mlp_init_kernel(const int32_t* __restrict__ feat_off, MlpNet net, int first,
                                                          const double* __restrict__ scale, unsigned long long seed, unsigned tag,
                                                          float* __restrict__ state, const int64_t* __restrict__ s_off) {
    const unsigned long long b = (unsigned long long)first + blockIdx.y;
    const unsigned k0 = (unsigned)seed ^ (unsigned)b, k1 = (unsigned)(seed >> 32) ^ (unsigned)(b >> 32) ^ 0x5bd1e995u;
    const int ds = feat_off[b + 1] - feat_off[b];
    float* out = state + s_off[blockIdx.y];
    int K = ds;
    for (int l = 0; l < net.nl; ++l) {
        const int N = mlp_outputs<O>(net, l, ds);
        const long weights = (long)N * K, total = O::kBias ? weights + N : weights;
        const double c = scale[(long)b * net.nl + l];
        for (long g = (long)blockIdx.x * kBlock + threadIdx.x; 4 * g < total; g += (long)gridDim.x * kBlock) {
            unsigned ctr[4] = {(unsigned)g, (unsigned)((unsigned long long)g >> 32), tag + (unsigned)l, 0u};
            philox4x32_10(ctr, k0, k1);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const long e = 4 * g + w;
                if (e < total) {
                    const double u = ((double)ctr[w] + 0.5) * 0x1p-32;  // exact
                    const long at = !O::kBias || e < weights ? (e % K) * N + e / K : e;
                    out[at] = (float)((2.0 * u - 1.0) * c);
                }
            }
        }
        out += total;
        K = N;
    }
}

template <class O>
static int mlp_init(MlpSite at, const int32_t* feat_off, int first, int count, int n_hidden, const int32_t* hidden, const double* scale,
                    uint64_t seed, unsigned tag, float* state, const int64_t* s_off, int64_t total, vgan_stream_t stream) {
    MlpNet net;
    VGAN_CHECK_ARG_AT(at.file, at.line, feat_off && scale && state && s_off && first >= 0 && count > 0 && count <= 65535 && total > 0);
    VGAN_CHECK_ARG_AT(at.file, at.line, mlp_net(n_hidden, hidden, VGAN_AE_ACT_RELU, O::kMirrored, &net));
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(state, 0, (size_t)total * sizeof(float), st) != hipSuccess) {  // the moments
        set_error("%s:%d: hipMemsetAsync failed", at.file, at.line);
        (void)hipGetLastError();
        return VGAN_ERR_HIP;
    }
    hipLaunchKernelGGL(mlp_init_kernel<O>, dim3(64, (unsigned)count), dim3(kBlock), 0, st, feat_off, net, first, scale,
                       (unsigned long long)seed, tag, state, s_off);
    VGAN_CHECK_LAUNCH_AT(at.file, at.line);
    return VGAN_OK;
}

// ---- the LDS-or-scratch launch ------------------------------------------------------------------------------------------
// kernel<true> with `floats` of dynamic LDS when they fit VGAN_AE_LDS_FLOATS (the attribute that allows it is set once per
// kernel), else kernel<false>, which works in a.scratch
template <auto KernelLds, auto KernelScratch, class Args>
static int mlp_launch(MlpSite at, dim3 grid, long floats, hipStream_t st, const Args& a, const MlpNet& net) {
    if (floats <= VGAN_AE_LDS_FLOATS) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KernelLds), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                           VGAN_AE_LDS_FLOATS * (int)sizeof(float));
        if (attr != hipSuccess) {
            set_error("%s:%d: hipFuncSetAttribute failed: %s", at.file, at.line, hipGetErrorString(attr));
            return VGAN_ERR_HIP;
        }
        hipLaunchKernelGGL(KernelLds, grid, dim3(kAeBlock), (size_t)floats * sizeof(float), st, a, net);
    } else {
        hipLaunchKernelGGL(KernelScratch, grid, dim3(kAeBlock), 0, st, a, net);
    }
    VGAN_CHECK_LAUNCH_AT(at.file, at.line);
    return VGAN_OK;
}

// ---- train --------------------------------------------------------------------------------------------------------------
struct MlpTrain {
    const float* X;
    long ldx;
    int n, w;  // rows; the half bits of feistel_perm for n
    const int32_t *feat, *feat_off;
    const double *mean, *scale;
    const int32_t* skip;
    int first, max_dims, batch, spe;  // spe: steps of an epoch, n / batch
    unsigned long long seed;
    long step_first;
    int step_count;
    const double* corr;  // [step_count][2]: 1 - beta1^t, 1 - beta2^t
    AeAdam adam;
    float* state;
    const int64_t* s_off;
    float* loss;
    long ld_loss;
    float* scratch;
    long scratch_stride;
    const float* center;  // [count][w] with O::kCenter, else null
};

template <bool LDS, class O>
__global__ __launch_bounds__(kAeBlock) void mlp_train_kernel(MlpTrain a, MlpNet net) {
    using P = std::conditional_t<LDS, ae_lds_f*, float*>;
    extern __shared__ __attribute__((aligned(16))) float mlp_lds_generic[];
    __shared__ int rowidx[VGAN_AE_MAX_BATCH];
    __shared__ float rowsum[VGAN_AE_MAX_BATCH];
    const int tid = threadIdx.x, s = a.first + (int)blockIdx.x;
    const int off = a.feat_off[s], ds = a.feat_off[s + 1] - off, B = a.batch;
    float* loss = a.loss + (long)blockIdx.x * a.ld_loss;
    if (ds > a.max_dims || a.skip[s]) {  // a constant subspace is not trained
        if (ds <= a.max_dims)
            for (int j = tid; j < a.step_count; j += kAeBlock) loss[a.step_first + j] = 0.f;
        return;
    }
    P base;
    if constexpr (LDS) base = (ae_lds_f*)mlp_lds_generic;
    else base = a.scratch + (long)blockIdx.x * a.scratch_stride;
    const int pz = ae_pitch(ds), pt = ae_pitch(net.wmax);
    // z, the output act[l] of every layer (pitch pact[l]), the error E of the last (pitch pe, width we), one passed-down error
    P z = base, act[O::kMaxLayers], E, down;
    int pact[O::kMaxLayers], pe;
    O::template place<P>(net, ds, B, z, pz, act, pact, E, pe, down);
    const int we = mlp_outputs<O>(net, net.nl - 1, ds);
    float* theta = a.state + a.s_off[blockIdx.x];
    const long P_n = mlp_params<O>(net, ds);
    long w_at[O::kMaxLayers];
    {
        long at = 0;
        int K = ds;
        for (int l = 0; l < O::kMaxLayers; ++l) {
            w_at[l] = at;
            if (l < net.nl) {
                const int N = mlp_outputs<O>(net, l, ds);
                at += (long)(K + (O::kBias ? 1 : 0)) * N;
                K = N;
            }
        }
    }
    ae_lds_f* cs = O::center_lds();
    if constexpr (O::kCenter)
        if (tid < we) cs[tid] = a.center[(long)blockIdx.x * we + tid];
    const int n_cells = O::loss_cells(B, ds);
    const float cells = (float)n_cells, two_inv = (float)(2.0 / (double)n_cells);
    for (int j = 0; j < a.step_count; ++j) {
        const long g = a.step_first + j;
        const unsigned long long epoch = (unsigned long long)(g / a.spe), i_step = (unsigned long long)(g % a.spe);
        const float lrc = (float)(a.adam.lr / a.corr[2 * j]), sc2 = (float)sqrt(a.corr[2 * j + 1]);
        if (tid < B) rowidx[tid] = (int)feistel_perm(i_step * (unsigned long long)B + tid, (unsigned long long)a.n, a.w, a.seed, epoch);
        __syncthreads();  // also: cs is written
        ae_stage<P>(a.X, a.ldx, rowidx, B, a.feat + off, a.mean, a.scale, ds, z, pz);
        __syncthreads();
        // forward; the last layer leaves r = out - target
        int K = ds;
        for (int l = 0; l < net.nl; ++l) {
            const int N = mlp_outputs<O>(net, l, ds);
            P in = l ? act[l - 1] : z, out = act[l];
            const int pin = l ? pact[l - 1] : pz, pout = pact[l];
            if (l + 1 < net.nl) {
                const int kind = net.act;
                ae_forward<O::kBias, P>(in, pin, K, theta + w_at[l], N, B, [&](int i, int o, float val) { out[i * pout + o] = ae_activate(val, kind); });
            } else {
                ae_forward<O::kBias, P>(in, pin, K, theta + w_at[l], N, B,
                                        [&](int i, int o, float val) { out[i * pout + o] = val - O::template target<P>(i, o, z, pz, cs); });
            }
            __syncthreads();
            K = N;
        }
        // the loss of the step, before its update, and the output error 2 r / cells
        if (tid < B) {
            P er = E + tid * pe;
            float sum = 0.f;
            for (int f = 0; f < we; ++f) {
                const float d = er[f];
                sum = fmaf(d, d, sum);
                er[f] = d * two_inv;
            }
            rowsum[tid] = sum;
        }
        __syncthreads();
        if (tid == 0) {
            float tot = 0.f;
            for (int i = 0; i < B; ++i) tot += rowsum[i];
            loss[g] = tot / cells;
        }
        // backward, from the last layer: K inputs, N outputs of layer l; its error is in act[l]
        for (int l = net.nl - 1; l >= 0; --l) {
            const int N = mlp_outputs<O>(net, l, ds), Kl = l ? net.width[l - 1] : ds;
            P in = l ? act[l - 1] : z;
            const int pin = l ? pact[l - 1] : pz;
            if (l) {
                ae_backprop<P>(act[l], pact[l], N, theta + w_at[l], Kl, B, down, pt);
                __syncthreads();  // the weights of layer l have been read as they were
            }
            ae_update<O::kBias, P>(act[l], pact[l], N, in, pin, Kl, B, theta + w_at[l], P_n, a.adam, lrc, sc2);
            __syncthreads();  // the inputs of layer l have been read as activations
            if (l) {
                ae_derivative<P>(in, pin, down, pt, Kl, B, net.act);
                __syncthreads();
            }
        }
    }
}

// The checks and the launch of a train entry (center: already checked by an entry that takes one, else null)
template <class O>
static int mlp_train(MlpSite at, const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                     const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden, const int32_t* hidden,
                     int activation, int batch, uint64_t seed, int64_t step_first, int step_count, const double* corr, double lr, double beta1,
                     double beta2, double eps, double weight_decay, const float* center, float* state, const int64_t* s_off, float* loss,
                     int64_t ld_loss, float* scratch, int64_t scratch_floats, vgan_stream_t stream) {
    MlpNet net;
    VGAN_CHECK_ARG_AT(at.file, at.line, X && feat && feat_off && mean && scale && skip && corr && state && s_off && loss && d > 0 &&
                                            ldx >= d);
    VGAN_CHECK_ARG_AT(at.file, at.line, n >= 2 && n <= VGAN_AE_MAX_ROWS && first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 &&
                                            max_dims <= VGAN_AE_MAX_DIMS);
    VGAN_CHECK_ARG_AT(at.file, at.line, mlp_net(n_hidden, hidden, activation, O::kMirrored, &net) && batch >= 1 &&
                                            batch <= VGAN_AE_MAX_BATCH && batch <= n);
    VGAN_CHECK_ARG_AT(at.file, at.line, step_first >= 0 && step_count >= 1 && step_count <= VGAN_AE_MAX_LAUNCH_STEPS &&
                                            ld_loss >= step_first + step_count);
    VGAN_CHECK_ARG_AT(at.file, at.line, lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0 && weight_decay >= 0.0);
    const long floats = mlp_act_floats<O>(net, max_dims, batch, true);
    VGAN_CHECK_ARG_AT(at.file, at.line, floats <= VGAN_AE_LDS_FLOATS || (scratch && scratch_floats >= floats * count));
    MlpTrain a;
    a.X = X, a.ldx = ldx, a.n = n, a.w = feistel_half_bits((unsigned long long)n), a.feat = feat, a.feat_off = feat_off;
    a.mean = mean, a.scale = scale, a.skip = skip, a.first = first, a.max_dims = max_dims, a.batch = batch, a.spe = n / batch;
    a.seed = seed, a.step_first = step_first, a.step_count = step_count, a.corr = corr;
    a.adam.b1 = (float)beta1, a.adam.omb1 = (float)(1.0 - beta1), a.adam.b2 = (float)beta2, a.adam.omb2 = (float)(1.0 - beta2);
    a.adam.eps = (float)eps, a.adam.wd = (float)weight_decay, a.adam.lr = lr;
    a.center = center, a.state = state, a.s_off = s_off, a.loss = loss, a.ld_loss = ld_loss, a.scratch = scratch, a.scratch_stride = floats;
    return mlp_launch<&mlp_train_kernel<true, O>, &mlp_train_kernel<false, O>>(at, dim3((unsigned)count), floats, (hipStream_t)stream, a, net);
}

// ---- forward ------------------------------------------------------------------------------------------------------------
struct MlpScore {
    const float* X;
    long ldx;
    int rows;
    const int32_t *feat, *feat_off;
    const double *mean, *scale;
    const int32_t* skip;
    int first, max_dims;
    const float* state;
    const int64_t* s_off;
    const float* center;  // [count][w]: the score mode of an objective with a centre
    float* score;
    long ld_score;
    float* raw;    // [rows][w]: the raw output of one block instead of scores
    double* tsum;  // [count][tiles][w]: the column sums of every row tile instead of scores
    float* scratch;
    long scratch_stride;
};

template <bool LDS, class O>
__global__ __launch_bounds__(kAeBlock) void mlp_forward_kernel(MlpScore a, MlpNet net) {
    using P = std::conditional_t<LDS, ae_lds_f*, float*>;
    extern __shared__ __attribute__((aligned(16))) float mlp_lds_generic[];
    __shared__ int rowidx[kAeRows];
    const int tid = threadIdx.x, s = a.first + (int)blockIdx.y, row0 = (int)blockIdx.x * kAeRows;
    const int off = a.feat_off[s], ds = a.feat_off[s + 1] - off, B = min(kAeRows, a.rows - row0);
    if (ds > a.max_dims) return;
    const int wo = mlp_outputs<O>(net, net.nl - 1, ds);
    double* tsum = O::kCenter && a.tsum ? a.tsum + ((long)blockIdx.y * gridDim.x + blockIdx.x) * wo : nullptr;
    if (!a.raw && a.skip[s]) {  // a constant subspace scores exactly 0 and has a centre of zeros
        if (tsum) {
            if (tid < wo) tsum[tid] = 0.0;
        } else if (tid < B) {
            a.score[(long)blockIdx.y * a.ld_score + row0 + tid] = 0.f;
        }
        return;
    }
    P base;
    if constexpr (LDS) base = (ae_lds_f*)mlp_lds_generic;
    else base = a.scratch + ((long)blockIdx.y * gridDim.x + blockIdx.x) * a.scratch_stride;
    const int pz = ae_pitch(ds);
    P z = base, at = z + kAeRows * pz;
    if (tid < B) rowidx[tid] = row0 + tid;
    __syncthreads();
    ae_stage<P>(a.X, a.ldx, rowidx, B, a.feat + off, a.mean, a.scale, ds, z, pz);
    __syncthreads();
    const float* Wl = a.state + a.s_off[blockIdx.y];
    P in = z;
    int pin = pz, K = ds;
    for (int l = 0; l < net.nl; ++l) {
        const int N = mlp_outputs<O>(net, l, ds);
        if (l + 1 < net.nl) {
            P out = at;
            const int pout = ae_pitch(N), kind = net.act;
            ae_forward<O::kBias, P>(in, pin, K, Wl, N, B, [&](int i, int o, float val) { out[i * pout + o] = ae_activate(val, kind); });
            in = out, pin = pout, at += kAeRows * pout;
        } else {  // into `at` if the objective keeps the output
            O::template last_layer<P>(a, in, pin, K, Wl, N, B, row0, z, pz, at);
        }
        __syncthreads();
        Wl += (long)(K + (O::kBias ? 1 : 0)) * N;
        K = N;
    }
    O::template finish<P>(a, B, row0, z, pz, at, wo, tsum);
}

// The checks every forward entry shares; fills the net, the row tiles and what of `a` does not depend on the mode (center,
// score, ld_score, raw and tsum are left null for the entry to set)
template <class O>
static int mlp_forward_args(MlpSite at, const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                            const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden, const int32_t* hidden,
                            int activation, const float* state, const int64_t* s_off, float* scratch, int64_t scratch_floats, MlpScore* a,
                            MlpNet* net, long* tiles) {
    VGAN_CHECK_ARG_AT(at.file, at.line, X && feat && feat_off && mean && scale && skip && state && s_off && d > 0 && ldx >= d);
    VGAN_CHECK_ARG_AT(at.file, at.line, rows >= 1 && rows <= VGAN_AE_MAX_ROWS && first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 &&
                                            max_dims <= VGAN_AE_MAX_DIMS);
    VGAN_CHECK_ARG_AT(at.file, at.line, mlp_net(n_hidden, hidden, activation, O::kMirrored, net));
    const long floats = mlp_act_floats<O>(*net, max_dims, kAeRows, false);
    *tiles = (rows + kAeRows - 1) / kAeRows;
    VGAN_CHECK_ARG_AT(at.file, at.line, floats <= VGAN_AE_LDS_FLOATS || (scratch && scratch_floats >= floats * *tiles * count));
    *a = MlpScore{};
    a->X = X, a->ldx = ldx, a->rows = rows, a->feat = feat, a->feat_off = feat_off, a->mean = mean, a->scale = scale, a->skip = skip;
    a->first = first, a->max_dims = max_dims, a->state = state, a->s_off = s_off, a->scratch = scratch, a->scratch_stride = floats;
    return VGAN_OK;
}

// the launch of a forward entry over `tiles` row tiles of `count` blocks
template <class O>
static int mlp_forward_launch(MlpSite at, const MlpScore& a, const MlpNet& net, int count, long tiles, hipStream_t st) {
    const dim3 grid((unsigned)tiles, (unsigned)count);
    return mlp_launch<&mlp_forward_kernel<true, O>, &mlp_forward_kernel<false, O>>(at, grid, a.scratch_stride, st, a, net);
}

}  // namespace vgan

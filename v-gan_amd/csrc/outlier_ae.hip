// Autoencoder outlier scores over the subspaces (pyod's AutoEncoder up to dropout and batch normalisation): one small MLP per
// subspace, trained by Adam on mini-batches to reconstruct the standardised rows through a bottleneck; a row is scored by the
// Euclidean norm of its reconstruction error.  v-gan_amd/outlier.py: SubspaceAutoEncoder, whose docstring is the definition.
// Block b = the subspace at position b.  Its net has the layer sizes K_0 = d_s, h_1 .. h_L, h_{L-1} .. h_1, d_s (nl = 2 L
// layers), a bias in every layer, the activation after every layer but the last.
//
//   state      of a block: theta, m, v, P floats each (P = sum_l (K_l + 1) N_l), one after the other.  Inside each, layer after
//              layer, W_l K-MAJOR as [K_l][N_l] (W_l[o, i] at i N_l + o), then b_l [N_l]: the bias is row K_l of the same image
//              (its input is the constant 1), so the forward reads it and the update walks it without a second rule.  The 64
//              lanes of a wave that compute 64 neighbouring outputs read 256 contiguous bytes of every k.
//   init       W_l[o, i] and b_l[o] from the Philox4x32-10 words of counter (e >> 2, 0, 0x41450000 + l, 0), e = o K_l + i, the
//              biases at e = N_l K_l + o, key (lo32(seed) ^ lo32(b), hi32(seed) ^ hi32(b) ^ 0x5bd1e995): word e & 3 is w, u = (w
//              + 0.5) 2^-32 in float64, value float32((2 u - 1) c_l), c_l = 1 / sqrt(K_l) from the host.  m = v = 0.
//   train      ONE WORKGROUP OWNS ONE NET FOR THE WHOLE LAUNCH and runs step after step: the batch rows (feistel_perm) are
//              gathered from X through the feature list and standardised while staged; the forward keeps every activation of
//              the batch; the output error, the loss; then layer by layer from the last: the error of the layer below through
//              the weights as they still are, the weight-gradient products with Adam behind each element (the gradient is a
//              register), the derivative of the activation.  Workgroups never wait for each other.  The activations live in
//              LDS while B (2 pitch(d_s) + sum pitch(h) + pitch(max h)) floats fit VGAN_AE_LDS_FLOATS, else in a slice of a
//              scratch buffer in global memory that only its own workgroup touches (it stays in L2): the same code through
//              the other address space, the same bits.
//   scores     one workgroup per (block, tile of VGAN_AE_ROW_TILE = 32 rows) runs the forward through the same layer routine
//              and sums the squared error per row in float64, features ascending; or writes the raw output (reconstruct).
//   values     every product is ONE chain of fmaf in ascending order of the summation index, starting from 0: over k for a
//              unit (then the bias is added), over the output units f for an error passed down, over the batch rows i for a
//              gradient.  A chain belongs to one thread, so no value depends on the launch, the chunk, the address space of
//              the activations or which other blocks share the launch.
// The layer routines (ae_stage, ae_forward, ae_backprop, ae_update, ae_adam, ae_activate, the pitch rule) live in
// outlier_mlp.hpp, shared with the Deep SVDD encoders of outlier_svdd.hip; this file instantiates them with a bias.
#include <type_traits>

#include "optim_common.hpp"
#include "outlier_mlp.hpp"
#include "vgan_common.hpp"

namespace vgan {

constexpr int kAeMaxLayers = 2 * VGAN_AE_MAX_HIDDEN;
constexpr unsigned kAePhiloxTag = 0x41450000u;  // "AE\0\0" + the layer: counter word 2

struct AeNet {
    int nl;                    // layers: 2 L
    int width[kAeMaxLayers];   // outputs of layer l < nl - 1; the last layer has d_s
    int act;                   // VGAN_AE_ACT_*
    int wmax;                  // the widest hidden layer
};

__host__ __device__ inline int ae_outputs(const AeNet& net, int l, int ds) { return l == net.nl - 1 ? ds : net.width[l]; }
__host__ __device__ inline long ae_params(const AeNet& net, int ds) {
    long p = 0;
    int K = ds;
    for (int l = 0; l < net.nl; ++l) {
        const int N = ae_outputs(net, l, ds);
        p += (long)(K + 1) * N;
        K = N;
    }
    return p;
}
// floats of the activations of `rows` rows: z, the hidden layers and, when training, the output error and one passed-down error
__host__ __device__ inline long ae_act_floats(const AeNet& net, int ds, int rows, bool train) {
    long f = (long)ae_pitch(ds) * (train ? 2 : 1) + (train ? ae_pitch(net.wmax) : 0);
    for (int l = 0; l + 1 < net.nl; ++l) f += ae_pitch(net.width[l]);
    return f * rows;
}

__global__ __launch_bounds__(kBlock) void ae_init_kernel(const int32_t* __restrict__ feat_off, AeNet net, int first,
                                                         const double* __restrict__ scale, unsigned long long seed,
                                                         float* __restrict__ state, const int64_t* __restrict__ s_off) {
    const unsigned long long b = (unsigned long long)first + blockIdx.y;
    const unsigned k0 = (unsigned)seed ^ (unsigned)b, k1 = (unsigned)(seed >> 32) ^ (unsigned)(b >> 32) ^ 0x5bd1e995u;
    const int ds = feat_off[b + 1] - feat_off[b];
    float* out = state + s_off[blockIdx.y];
    int K = ds;
    for (int l = 0; l < net.nl; ++l) {
        const int N = ae_outputs(net, l, ds);
        const long weights = (long)N * K, total = weights + N;
        const double c = scale[(long)b * net.nl + l];
        for (long g = (long)blockIdx.x * kBlock + threadIdx.x; 4 * g < total; g += (long)gridDim.x * kBlock) {
            unsigned ctr[4] = {(unsigned)g, (unsigned)((unsigned long long)g >> 32), kAePhiloxTag + (unsigned)l, 0u};
            philox4x32_10(ctr, k0, k1);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const long e = 4 * g + w;
                if (e < total) {
                    const double u = ((double)ctr[w] + 0.5) * 0x1p-32;  // exact
                    const long at = e < weights ? (e % K) * N + e / K : e;
                    out[at] = (float)((2.0 * u - 1.0) * c);
                }
            }
        }
        out += total;
        K = N;
    }
}

struct AeTrain {
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
};

template <bool LDS>
__global__ __launch_bounds__(kAeBlock) void ae_train_kernel(AeTrain a, AeNet net) {
    using P = std::conditional_t<LDS, ae_lds_f*, float*>;
    extern __shared__ __attribute__((aligned(16))) float ae_lds_generic[];
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
    if constexpr (LDS) base = (ae_lds_f*)ae_lds_generic;
    else base = a.scratch + (long)blockIdx.x * a.scratch_stride;
    const int pz = ae_pitch(ds), pt = ae_pitch(net.wmax);
    P z = base, E = z + B * pz, act[kAeMaxLayers];
    int pact[kAeMaxLayers];
    {
        P at = E + B * pz;
        for (int l = 0; l + 1 < net.nl; ++l) {
            act[l] = at, pact[l] = ae_pitch(net.width[l]);
            at += B * pact[l];
        }
        act[net.nl - 1] = E, pact[net.nl - 1] = pz;
        for (int l = net.nl; l < kAeMaxLayers; ++l) act[l] = E, pact[l] = pz;
    }
    P down = act[net.nl - 2] + B * pact[net.nl - 2];
    float* theta = a.state + a.s_off[blockIdx.x];
    const long P_n = ae_params(net, ds);
    long w_at[kAeMaxLayers];
    {
        long at = 0;
        int K = ds;
        for (int l = 0; l < kAeMaxLayers; ++l) {
            w_at[l] = at;
            if (l < net.nl) {
                const int N = ae_outputs(net, l, ds);
                at += (long)(K + 1) * N;
                K = N;
            }
        }
    }
    const float cells = (float)(B * ds), two_inv = (float)(2.0 / (double)(B * ds));
    for (int j = 0; j < a.step_count; ++j) {
        const long g = a.step_first + j;
        const unsigned long long epoch = (unsigned long long)(g / a.spe), i_step = (unsigned long long)(g % a.spe);
        const float lrc = (float)(a.adam.lr / a.corr[2 * j]), sc2 = (float)sqrt(a.corr[2 * j + 1]);
        if (tid < B) rowidx[tid] = (int)feistel_perm(i_step * (unsigned long long)B + tid, (unsigned long long)a.n, a.w, a.seed, epoch);
        __syncthreads();
        ae_stage<P>(a.X, a.ldx, rowidx, B, a.feat + off, a.mean, a.scale, ds, z, pz);
        __syncthreads();
        // forward
        int K = ds;
        for (int l = 0; l < net.nl; ++l) {
            const int N = ae_outputs(net, l, ds);
            P in = l ? act[l - 1] : z, out = act[l];
            const int pin = l ? pact[l - 1] : pz, pout = pact[l];
            if (l + 1 < net.nl) {
                const int kind = net.act;
                ae_forward<true, P>(in, pin, K, theta + w_at[l], N, B, [&](int i, int o, float val) { out[i * pout + o] = ae_activate(val, kind); });
            } else {
                ae_forward<true, P>(in, pin, K, theta + w_at[l], N, B, [&](int i, int o, float val) { out[i * pout + o] = val - z[i * pz + o]; });
            }
            __syncthreads();
            K = N;
        }
        // the loss of the step, before its update, and the output error 2 (out - z) / (B d_s)
        if (tid < B) {
            P er = E + tid * pz;
            float sum = 0.f;
            for (int f = 0; f < ds; ++f) {
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
            const int N = ae_outputs(net, l, ds), Kl = l ? net.width[l - 1] : ds;
            P in = l ? act[l - 1] : z;
            const int pin = l ? pact[l - 1] : pz;
            if (l) {
                ae_backprop<P>(act[l], pact[l], N, theta + w_at[l], Kl, B, down, pt);
                __syncthreads();  // the weights of layer l have been read as they were
            }
            ae_update<true, P>(act[l], pact[l], N, in, pin, Kl, B, theta + w_at[l], P_n, a.adam, lrc, sc2);
            __syncthreads();  // the inputs of layer l have been read as activations
            if (l) {
                ae_derivative<P>(in, pin, down, pt, Kl, B, net.act);
                __syncthreads();
            }
        }
    }
}

struct AeScore {
    const float* X;
    long ldx;
    int rows;
    const int32_t *feat, *feat_off;
    const double *mean, *scale;
    const int32_t* skip;
    int first, max_dims;
    const float* state;
    const int64_t* s_off;
    float* score;
    long ld_score;
    float* recon;
    float* scratch;
    long scratch_stride;
};

template <bool LDS>
__global__ __launch_bounds__(kAeBlock) void ae_scores_kernel(AeScore a, AeNet net) {
    using P = std::conditional_t<LDS, ae_lds_f*, float*>;
    extern __shared__ __attribute__((aligned(16))) float ae_lds_generic[];
    __shared__ int rowidx[kAeRows];
    const int tid = threadIdx.x, s = a.first + (int)blockIdx.y, row0 = (int)blockIdx.x * kAeRows;
    const int off = a.feat_off[s], ds = a.feat_off[s + 1] - off, B = min(kAeRows, a.rows - row0);
    if (ds > a.max_dims) return;
    if (!a.recon && a.skip[s]) {  // a constant subspace scores exactly 0
        if (tid < B) a.score[(long)blockIdx.y * a.ld_score + row0 + tid] = 0.f;
        return;
    }
    P base;
    if constexpr (LDS) base = (ae_lds_f*)ae_lds_generic;
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
        const int N = ae_outputs(net, l, ds);
        if (l + 1 < net.nl) {
            P out = at;
            const int pout = ae_pitch(N), kind = net.act;
            ae_forward<true, P>(in, pin, K, Wl, N, B, [&](int i, int o, float val) { out[i * pout + o] = ae_activate(val, kind); });
            in = out, pin = pout, at += kAeRows * pout;
        } else if (a.recon) {
            float* R = a.recon + (long)row0 * ds;
            ae_forward<true, P>(in, pin, K, Wl, N, B, [&](int i, int o, float val) { R[(long)i * ds + o] = val; });
        } else {  // z has been read by layer 0 only: the error takes its place
            ae_forward<true, P>(in, pin, K, Wl, N, B, [&](int i, int o, float val) { z[i * pz + o] = val - z[i * pz + o]; });
        }
        __syncthreads();
        Wl += (long)(K + 1) * N;
        K = N;
    }
    if (!a.recon && tid < B) {
        P er = z + tid * pz;
        double sum = 0.0;
        for (int f = 0; f < ds; ++f) {
            const double d = (double)er[f];
            sum += d * d;  // the square of a float32 is exact in float64
        }
        a.score[(long)blockIdx.y * a.ld_score + row0 + tid] = (float)sqrt(sum);
    }
}

}  // namespace vgan

using namespace vgan;

// the net of the arguments; false when a size is out of range
static bool ae_net(int n_hidden, const int32_t* hidden, int activation, AeNet* net) {
    if (n_hidden < 1 || n_hidden > VGAN_AE_MAX_HIDDEN || !hidden) return false;
    if (activation != VGAN_AE_ACT_TANH && activation != VGAN_AE_ACT_RELU) return false;
    net->nl = 2 * n_hidden;
    net->wmax = 0;
    for (int l = 0; l < kAeMaxLayers; ++l) net->width[l] = 0;
    for (int l = 0; l < n_hidden; ++l) {
        if (hidden[l] < 1 || hidden[l] > VGAN_AE_MAX_WIDTH) return false;
        net->width[l] = net->width[2 * n_hidden - 2 - l] = hidden[l];
        if (hidden[l] > net->wmax) net->wmax = hidden[l];
    }
    net->act = activation;
    return true;
}

extern "C" int vgan_ae_init(const int32_t* feat_off, int first, int count, int n_hidden, const int32_t* hidden, const double* scale,
                            uint64_t seed, float* state, const int64_t* s_off, int64_t total, vgan_stream_t stream) {
    AeNet net;
    VGAN_CHECK_ARG(feat_off && scale && state && s_off && first >= 0 && count > 0 && count <= 65535 && total > 0);
    VGAN_CHECK_ARG(ae_net(n_hidden, hidden, VGAN_AE_ACT_RELU, &net));
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(state, 0, (size_t)total * sizeof(float), st) != hipSuccess) {  // the moments
        set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        (void)hipGetLastError();
        return VGAN_ERR_HIP;
    }
    hipLaunchKernelGGL(ae_init_kernel, dim3(64, (unsigned)count), dim3(kBlock), 0, st, feat_off, net, first, scale, (unsigned long long)seed,
                       state, s_off);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ae_train(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                             const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                             const int32_t* hidden, int activation, int batch, uint64_t seed, int64_t step_first, int step_count,
                             const double* corr, double lr, double beta1, double beta2, double eps, double weight_decay, float* state,
                             const int64_t* s_off, float* loss, int64_t ld_loss, float* scratch, int64_t scratch_floats,
                             vgan_stream_t stream) {
    AeNet net;
    VGAN_CHECK_ARG(X && feat && feat_off && mean && scale && skip && corr && state && s_off && loss && d > 0 && ldx >= d);
    VGAN_CHECK_ARG(n >= 2 && n <= VGAN_AE_MAX_ROWS && first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 && max_dims <= VGAN_AE_MAX_DIMS);
    VGAN_CHECK_ARG(ae_net(n_hidden, hidden, activation, &net) && batch >= 1 && batch <= VGAN_AE_MAX_BATCH && batch <= n);
    VGAN_CHECK_ARG(step_first >= 0 && step_count >= 1 && step_count <= VGAN_AE_MAX_LAUNCH_STEPS && ld_loss >= step_first + step_count);
    VGAN_CHECK_ARG(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0 && weight_decay >= 0.0);
    const long floats = ae_act_floats(net, max_dims, batch, true);
    const bool lds = floats <= VGAN_AE_LDS_FLOATS;
    VGAN_CHECK_ARG(lds || (scratch && scratch_floats >= floats * count));
    AeTrain a;
    a.X = X, a.ldx = ldx, a.n = n, a.w = feistel_half_bits((unsigned long long)n), a.feat = feat, a.feat_off = feat_off;
    a.mean = mean, a.scale = scale, a.skip = skip, a.first = first, a.max_dims = max_dims, a.batch = batch, a.spe = n / batch;
    a.seed = seed, a.step_first = step_first, a.step_count = step_count, a.corr = corr;
    a.adam.b1 = (float)beta1, a.adam.omb1 = (float)(1.0 - beta1), a.adam.b2 = (float)beta2, a.adam.omb2 = (float)(1.0 - beta2);
    a.adam.eps = (float)eps, a.adam.wd = (float)weight_decay, a.adam.lr = lr;
    a.state = state, a.s_off = s_off, a.loss = loss, a.ld_loss = ld_loss, a.scratch = scratch, a.scratch_stride = floats;
    const hipStream_t st = (hipStream_t)stream;
    if (lds) {
        static const int allowed = ae_allow_lds(&ae_train_kernel<true>, __FILE__, __LINE__);
        if (allowed != VGAN_OK) return allowed;
        hipLaunchKernelGGL(ae_train_kernel<true>, dim3((unsigned)count), dim3(kAeBlock), (size_t)floats * sizeof(float), st, a, net);
    } else {
        hipLaunchKernelGGL(ae_train_kernel<false>, dim3((unsigned)count), dim3(kAeBlock), 0, st, a, net);
    }
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_ae_scores(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                              const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                              const int32_t* hidden, int activation, const float* state, const int64_t* s_off, float* score,
                              int64_t ld_score, float* recon, float* scratch, int64_t scratch_floats, vgan_stream_t stream) {
    AeNet net;
    VGAN_CHECK_ARG(X && feat && feat_off && mean && scale && skip && state && s_off && d > 0 && ldx >= d);
    VGAN_CHECK_ARG(rows >= 1 && rows <= VGAN_AE_MAX_ROWS && first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 && max_dims <= VGAN_AE_MAX_DIMS);
    VGAN_CHECK_ARG(ae_net(n_hidden, hidden, activation, &net));
    VGAN_CHECK_ARG(recon ? count == 1 : (score && ld_score >= rows));
    const long floats = ae_act_floats(net, max_dims, kAeRows, false);
    const bool lds = floats <= VGAN_AE_LDS_FLOATS;
    const long tiles = (rows + kAeRows - 1) / kAeRows;
    VGAN_CHECK_ARG(lds || (scratch && scratch_floats >= floats * tiles * count));
    AeScore a;
    a.X = X, a.ldx = ldx, a.rows = rows, a.feat = feat, a.feat_off = feat_off, a.mean = mean, a.scale = scale, a.skip = skip;
    a.first = first, a.max_dims = max_dims, a.state = state, a.s_off = s_off, a.score = score, a.ld_score = ld_score, a.recon = recon;
    a.scratch = scratch, a.scratch_stride = floats;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)count);
    if (lds) {
        static const int allowed = ae_allow_lds(&ae_scores_kernel<true>, __FILE__, __LINE__);
        if (allowed != VGAN_OK) return allowed;
        hipLaunchKernelGGL(ae_scores_kernel<true>, grid, dim3(kAeBlock), (size_t)floats * sizeof(float), st, a, net);
    } else {
        hipLaunchKernelGGL(ae_scores_kernel<false>, grid, dim3(kAeBlock), 0, st, a, net);
    }
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

// Deep SVDD one-class scores over the subspaces (Ruff et al. 2018; pyod's DeepSVDD, the one-class objective): one small encoder
// per subspace, trained by Adam on mini-batches to map the standardised rows onto one point c; a row is scored by the squared
// distance of its image from c.  v-gan_amd/outlier.py: SubspaceDeepSVDD, whose docstring is the definition.
// Block b = the subspace at position b.  Its net has the layer sizes K_0 = d_s, h_1 .. h_L (nl = L layers), NO BIAS anywhere,
// the activation after every layer but the last; q = h_L is the output dimension.
//
//   state      of a block: theta, m, v, P floats each (P = sum_l K_l N_l), one after the other.  Inside each, layer after
//              layer, W_l K-MAJOR as [K_l][N_l] (W_l[o, i] at i N_l + o): the autoencoder's image without the bias row.
//   init       W_l[o, i] from the Philox4x32-10 words of counter (e >> 2, 0, 0x53564400 + l, 0), e = o K_l + i, under the
//              autoencoder's key and value rule.  m = v = 0.
//   centre     the forward of the untrained net over all fitted rows: one workgroup per (block, 32-row tile) sums its outputs
//              per coordinate in float64, rows ascending; a second kernel adds the tile sums to a running float64 sum in tile
//              order and, after the last chunk of rows, divides by n, applies the center_eps rule and rounds to float32.
//   train      the autoencoder's loop (one workgroup owns one net for the whole launch, activations in LDS or in a private
//              scratch slice) with the error r = out - c, the loss sum r^2 / B and the output error r float32(2 / B).
//   scores     one workgroup per (block, tile of 32 rows): float32(sum_j double(out_j - c_j)^2), j ascending; or the raw
//              output (embed).
// The layer routines are those of outlier_mlp.hpp, instantiated without a bias.
#include <type_traits>

#include "optim_common.hpp"
#include "outlier_mlp.hpp"
#include "vgan_common.hpp"

namespace vgan {

constexpr int kSvddMaxLayers = VGAN_AE_MAX_HIDDEN;
constexpr unsigned kSvddPhiloxTag = VGAN_SVDD_PHILOX_TAG;  // "SVD\0" + the layer: counter word 2
constexpr int kSvddFold = VGAN_SVDD_MAX_OUT;               // threads of the fold kernel: one per output coordinate

struct SvddNet {
    int nl;                     // layers: L
    int width[kSvddMaxLayers];  // outputs of layer l; the last is q
    int act;                    // VGAN_AE_ACT_*
    int wmax;                   // the widest layer
};

__host__ __device__ inline long svdd_params(const SvddNet& net, int ds) {
    long p = 0;
    int K = ds;
    for (int l = 0; l < net.nl; ++l) {
        p += (long)K * net.width[l];
        K = net.width[l];
    }
    return p;
}
// floats of the activations of `rows` rows: z, every layer's output and, when training, one passed-down error
__host__ __device__ inline long svdd_act_floats(const SvddNet& net, int ds, int rows, bool train) {
    long f = (long)ae_pitch(ds) + (train ? ae_pitch(net.wmax) : 0);
    for (int l = 0; l < net.nl; ++l) f += ae_pitch(net.width[l]);
    return f * rows;
}

__global__ __launch_bounds__(kBlock) void svdd_init_kernel(const int32_t* __restrict__ feat_off, SvddNet net, int first,
                                                           const double* __restrict__ scale, unsigned long long seed,
                                                           float* __restrict__ state, const int64_t* __restrict__ s_off) {
    const unsigned long long b = (unsigned long long)first + blockIdx.y;
    const unsigned k0 = (unsigned)seed ^ (unsigned)b, k1 = (unsigned)(seed >> 32) ^ (unsigned)(b >> 32) ^ 0x5bd1e995u;
    const int ds = feat_off[b + 1] - feat_off[b];
    float* out = state + s_off[blockIdx.y];
    int K = ds;
    for (int l = 0; l < net.nl; ++l) {
        const int N = net.width[l];
        const long total = (long)N * K;
        const double c = scale[(long)b * net.nl + l];
        for (long g = (long)blockIdx.x * kBlock + threadIdx.x; 4 * g < total; g += (long)gridDim.x * kBlock) {
            unsigned ctr[4] = {(unsigned)g, (unsigned)((unsigned long long)g >> 32), kSvddPhiloxTag + (unsigned)l, 0u};
            philox4x32_10(ctr, k0, k1);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const long e = 4 * g + w;
                if (e < total) {
                    const double u = ((double)ctr[w] + 0.5) * 0x1p-32;  // exact
                    out[(e % K) * N + e / K] = (float)((2.0 * u - 1.0) * c);
                }
            }
        }
        out += total;
        K = N;
    }
}

struct SvddTrain {
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
    const float* center;  // [count][q]
    float* state;
    const int64_t* s_off;
    float* loss;
    long ld_loss;
    float* scratch;
    long scratch_stride;
};

template <bool LDS>
__global__ __launch_bounds__(kAeBlock) void svdd_train_kernel(SvddTrain a, SvddNet net) {
    using P = std::conditional_t<LDS, ae_lds_f*, float*>;
    extern __shared__ __attribute__((aligned(16))) float svdd_lds_generic[];
    __shared__ int rowidx[VGAN_AE_MAX_BATCH];
    __shared__ float rowsum[VGAN_AE_MAX_BATCH];
    __shared__ float cs[VGAN_SVDD_MAX_OUT];
    const int tid = threadIdx.x, s = a.first + (int)blockIdx.x;
    const int off = a.feat_off[s], ds = a.feat_off[s + 1] - off, B = a.batch;
    float* loss = a.loss + (long)blockIdx.x * a.ld_loss;
    if (ds > a.max_dims || a.skip[s]) {  // a constant subspace is not trained
        if (ds <= a.max_dims)
            for (int j = tid; j < a.step_count; j += kAeBlock) loss[a.step_first + j] = 0.f;
        return;
    }
    P base;
    if constexpr (LDS) base = (ae_lds_f*)svdd_lds_generic;
    else base = a.scratch + (long)blockIdx.x * a.scratch_stride;
    const int L = net.nl, q = net.width[L - 1], pz = ae_pitch(ds), pt = ae_pitch(net.wmax);
    P z = base, act[kSvddMaxLayers];
    int pact[kSvddMaxLayers];
    long w_at[kSvddMaxLayers];
    P down;
    {
        P at = z + B * pz;
        long wat = 0;
        int K = ds;
        for (int l = 0; l < kSvddMaxLayers; ++l) {
            if (l < L) {
                act[l] = at, pact[l] = ae_pitch(net.width[l]), w_at[l] = wat;
                at += B * pact[l];
                wat += (long)K * net.width[l];
                K = net.width[l];
            } else {
                act[l] = act[L - 1], pact[l] = pact[L - 1], w_at[l] = 0;
            }
        }
        down = at;
    }
    float* theta = a.state + a.s_off[blockIdx.x];
    const long P_n = svdd_params(net, ds);
    if (tid < q) cs[tid] = a.center[(long)blockIdx.x * q + tid];
    const float rows_f = (float)B, two_inv = (float)(2.0 / (double)B);
    P E = act[L - 1];
    const int pq = pact[L - 1];
    for (int j = 0; j < a.step_count; ++j) {
        const long g = a.step_first + j;
        const unsigned long long epoch = (unsigned long long)(g / a.spe), i_step = (unsigned long long)(g % a.spe);
        const float lrc = (float)(a.adam.lr / a.corr[2 * j]), sc2 = (float)sqrt(a.corr[2 * j + 1]);
        if (tid < B) rowidx[tid] = (int)feistel_perm(i_step * (unsigned long long)B + tid, (unsigned long long)a.n, a.w, a.seed, epoch);
        __syncthreads();  // also: cs is written
        ae_stage<P>(a.X, a.ldx, rowidx, B, a.feat + off, a.mean, a.scale, ds, z, pz);
        __syncthreads();
        // forward; the last layer leaves r = out - c
        int K = ds;
        for (int l = 0; l < L; ++l) {
            const int N = net.width[l];
            P in = l ? act[l - 1] : z, out = act[l];
            const int pin = l ? pact[l - 1] : pz, pout = pact[l];
            if (l + 1 < L) {
                const int kind = net.act;
                ae_forward<false, P>(in, pin, K, theta + w_at[l], N, B, [&](int i, int o, float val) { out[i * pout + o] = ae_activate(val, kind); });
            } else {
                ae_forward<false, P>(in, pin, K, theta + w_at[l], N, B, [&](int i, int o, float val) { out[i * pout + o] = val - cs[o]; });
            }
            __syncthreads();
            K = N;
        }
        // the loss of the step, before its update, and the output error 2 (out - c) / B
        if (tid < B) {
            P er = E + tid * pq;
            float sum = 0.f;
            for (int f = 0; f < q; ++f) {
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
            loss[g] = tot / rows_f;
        }
        // backward, from the last layer: K inputs, N outputs of layer l; its error is in act[l]
        for (int l = L - 1; l >= 0; --l) {
            const int N = net.width[l], Kl = l ? net.width[l - 1] : ds;
            P in = l ? act[l - 1] : z;
            const int pin = l ? pact[l - 1] : pz;
            if (l) {
                ae_backprop<P>(act[l], pact[l], N, theta + w_at[l], Kl, B, down, pt);
                __syncthreads();  // the weights of layer l have been read as they were
            }
            ae_update<false, P>(act[l], pact[l], N, in, pin, Kl, B, theta + w_at[l], P_n, a.adam, lrc, sc2);
            __syncthreads();  // the inputs of layer l have been read as activations
            if (l) {
                ae_derivative<P>(in, pin, down, pt, Kl, B, net.act);
                __syncthreads();
            }
        }
    }
}

struct SvddScore {
    const float* X;
    long ldx;
    int rows;
    const int32_t *feat, *feat_off;
    const double *mean, *scale;
    const int32_t* skip;
    int first, max_dims;
    const float* state;
    const int64_t* s_off;
    const float* center;  // [count][q]: the score mode
    float* score;
    long ld_score;
    float* embed;  // [rows][q]: the raw output of one block
    double* tsum;  // [count][tiles][q]: the column sums of every row tile
    float* scratch;
    long scratch_stride;
};

template <bool LDS>
__global__ __launch_bounds__(kAeBlock) void svdd_scores_kernel(SvddScore a, SvddNet net) {
    using P = std::conditional_t<LDS, ae_lds_f*, float*>;
    extern __shared__ __attribute__((aligned(16))) float svdd_lds_generic[];
    __shared__ int rowidx[kAeRows];
    const int tid = threadIdx.x, s = a.first + (int)blockIdx.y, row0 = (int)blockIdx.x * kAeRows;
    const int off = a.feat_off[s], ds = a.feat_off[s + 1] - off, B = min(kAeRows, a.rows - row0);
    if (ds > a.max_dims) return;
    const int L = net.nl, q = net.width[L - 1];
    double* tsum = a.tsum ? a.tsum + ((long)blockIdx.y * gridDim.x + blockIdx.x) * q : nullptr;
    if (!a.embed && a.skip[s]) {  // a constant subspace scores exactly 0 and has a centre of zeros
        if (tsum) {
            if (tid < q) tsum[tid] = 0.0;
        } else if (tid < B) {
            a.score[(long)blockIdx.y * a.ld_score + row0 + tid] = 0.f;
        }
        return;
    }
    P base;
    if constexpr (LDS) base = (ae_lds_f*)svdd_lds_generic;
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
    for (int l = 0; l < L; ++l) {
        const int N = net.width[l];
        P out = at;
        const int pout = ae_pitch(N);
        if (l + 1 < L) {
            const int kind = net.act;
            ae_forward<false, P>(in, pin, K, Wl, N, B, [&](int i, int o, float val) { out[i * pout + o] = ae_activate(val, kind); });
        } else {
            ae_forward<false, P>(in, pin, K, Wl, N, B, [&](int i, int o, float val) { out[i * pout + o] = val; });
        }
        __syncthreads();
        in = out, pin = pout, at += kAeRows * pout;
        Wl += (long)K * N;
        K = N;
    }
    if (a.embed) {
        float* R = a.embed + (long)row0 * q;
        for (int idx = tid; idx < B * q; idx += kAeBlock) {
            const int i = idx / q, o = idx - i * q;
            R[(long)i * q + o] = in[i * pin + o];
        }
    } else if (tsum) {
        if (tid < q) {
            double sum = 0.0;
            for (int i = 0; i < B; ++i) sum += (double)in[i * pin + tid];
            tsum[tid] = sum;
        }
    } else if (tid < B) {
        const float* c = a.center + (long)blockIdx.y * q;
        P orow = in + tid * pin;
        double sum = 0.0;
        for (int f = 0; f < q; ++f) {
            const double d = (double)(orow[f] - c[f]);
            sum += d * d;  // the square of a float32 is exact in float64
        }
        a.score[(long)blockIdx.y * a.ld_score + row0 + tid] = (float)sum;
    }
}

// run[b][j] += the tile sums of the chunk in tile order; with n_total > 0 (the last chunk) the centre: the mean, the
// center_eps rule, the rounding to float32, and the number of clamped coordinates
__global__ __launch_bounds__(kSvddFold) void svdd_center_kernel(const double* __restrict__ tsum, int tiles, int q, double* __restrict__ run,
                                                                long n_total, double center_eps, const int32_t* __restrict__ skip, int first,
                                                                float* __restrict__ center, int32_t* __restrict__ n_clamped) {
    __shared__ int flag[kSvddFold];
    const int b = blockIdx.x, j = threadIdx.x;
    int clamped = 0;
    if (j < q) {
        double sum = run[(long)b * q + j];
        for (int t = 0; t < tiles; ++t) sum += tsum[((long)b * tiles + t) * q + j];
        run[(long)b * q + j] = sum;
        if (n_total > 0) {
            double mean = sum / (double)n_total;
            if (skip[first + b]) {
                mean = 0.0;
            } else if (center_eps > 0.0 && fabs(mean) < center_eps) {
                mean = mean < 0.0 ? -center_eps : center_eps;
                clamped = 1;
            }
            center[(long)b * q + j] = (float)mean;
        }
    }
    flag[j] = clamped;
    __syncthreads();
    if (j == 0 && n_total > 0) {
        int total = 0;
        for (int o = 0; o < q; ++o) total += flag[o];
        n_clamped[b] = total;
    }
}

}  // namespace vgan

using namespace vgan;

// the net of the arguments; false when a size is out of range
static bool svdd_net(int n_hidden, const int32_t* hidden, int activation, SvddNet* net) {
    if (n_hidden < 1 || n_hidden > VGAN_AE_MAX_HIDDEN || !hidden) return false;
    if (activation != VGAN_AE_ACT_TANH && activation != VGAN_AE_ACT_RELU) return false;
    net->nl = n_hidden;
    net->wmax = 0;
    for (int l = 0; l < kSvddMaxLayers; ++l) net->width[l] = 0;
    for (int l = 0; l < n_hidden; ++l) {
        if (hidden[l] < 1 || hidden[l] > VGAN_AE_MAX_WIDTH) return false;
        net->width[l] = hidden[l];
        if (hidden[l] > net->wmax) net->wmax = hidden[l];
    }
    net->act = activation;
    return true;
}

extern "C" int vgan_svdd_init(const int32_t* feat_off, int first, int count, int n_hidden, const int32_t* hidden, const double* scale,
                              uint64_t seed, float* state, const int64_t* s_off, int64_t total, vgan_stream_t stream) {
    SvddNet net;
    VGAN_CHECK_ARG(feat_off && scale && state && s_off && first >= 0 && count > 0 && count <= 65535 && total > 0);
    VGAN_CHECK_ARG(svdd_net(n_hidden, hidden, VGAN_AE_ACT_RELU, &net));
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(state, 0, (size_t)total * sizeof(float), st) != hipSuccess) {  // the moments
        set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        (void)hipGetLastError();
        return VGAN_ERR_HIP;
    }
    hipLaunchKernelGGL(svdd_init_kernel, dim3(64, (unsigned)count), dim3(kBlock), 0, st, feat_off, net, first, scale, (unsigned long long)seed,
                       state, s_off);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

// the forward launch shared by vgan_svdd_scores and vgan_svdd_center; the arguments have been checked
static int svdd_forward_launch(SvddScore& a, const SvddNet& net, int count, long floats, long tiles, hipStream_t st) {
    a.scratch_stride = floats;
    const dim3 grid((unsigned)tiles, (unsigned)count);
    if (floats <= VGAN_AE_LDS_FLOATS) {
        static const int allowed = ae_allow_lds(&svdd_scores_kernel<true>, __FILE__, __LINE__);
        if (allowed != VGAN_OK) return allowed;
        hipLaunchKernelGGL(svdd_scores_kernel<true>, grid, dim3(kAeBlock), (size_t)floats * sizeof(float), st, a, net);
    } else {
        hipLaunchKernelGGL(svdd_scores_kernel<false>, grid, dim3(kAeBlock), 0, st, a, net);
    }
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_svdd_center(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                                const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                                const int32_t* hidden, int activation, const float* state, const int64_t* s_off, double* tile_sums,
                                int64_t tile_cells, double* run_sums, int64_t n_total, double center_eps, float* center,
                                int32_t* n_clamped, float* scratch, int64_t scratch_floats, vgan_stream_t stream) {
    SvddNet net;
    VGAN_CHECK_ARG(X && feat && feat_off && mean && scale && skip && state && s_off && tile_sums && run_sums && d > 0 && ldx >= d);
    VGAN_CHECK_ARG(rows >= 1 && rows <= VGAN_AE_MAX_ROWS && first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 && max_dims <= VGAN_AE_MAX_DIMS);
    VGAN_CHECK_ARG(svdd_net(n_hidden, hidden, activation, &net));
    VGAN_CHECK_ARG(n_total >= 0 && n_total <= VGAN_AE_MAX_ROWS && center_eps >= 0.0 && (n_total == 0 || (center && n_clamped)));
    const int q = net.width[net.nl - 1];
    const long floats = svdd_act_floats(net, max_dims, kAeRows, false);
    const long tiles = (rows + kAeRows - 1) / kAeRows;
    VGAN_CHECK_ARG(tile_cells >= tiles * count * q);
    VGAN_CHECK_ARG(floats <= VGAN_AE_LDS_FLOATS || (scratch && scratch_floats >= floats * tiles * count));
    SvddScore a;
    a.X = X, a.ldx = ldx, a.rows = rows, a.feat = feat, a.feat_off = feat_off, a.mean = mean, a.scale = scale, a.skip = skip;
    a.first = first, a.max_dims = max_dims, a.state = state, a.s_off = s_off, a.center = nullptr, a.score = nullptr, a.ld_score = 0;
    a.embed = nullptr, a.tsum = tile_sums, a.scratch = scratch;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = svdd_forward_launch(a, net, count, floats, tiles, st);
    if (rc != VGAN_OK) return rc;
    hipLaunchKernelGGL(svdd_center_kernel, dim3((unsigned)count), dim3(kSvddFold), 0, st, tile_sums, (int)tiles, q, run_sums, (long)n_total,
                       center_eps, skip, first, center, n_clamped);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_svdd_train(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                               const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                               const int32_t* hidden, int activation, int batch, uint64_t seed, int64_t step_first, int step_count,
                               const double* corr, double lr, double beta1, double beta2, double eps, double weight_decay,
                               const float* center, float* state, const int64_t* s_off, float* loss, int64_t ld_loss, float* scratch,
                               int64_t scratch_floats, vgan_stream_t stream) {
    SvddNet net;
    VGAN_CHECK_ARG(X && feat && feat_off && mean && scale && skip && corr && center && state && s_off && loss && d > 0 && ldx >= d);
    VGAN_CHECK_ARG(n >= 2 && n <= VGAN_AE_MAX_ROWS && first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 && max_dims <= VGAN_AE_MAX_DIMS);
    VGAN_CHECK_ARG(svdd_net(n_hidden, hidden, activation, &net) && batch >= 1 && batch <= VGAN_AE_MAX_BATCH && batch <= n);
    VGAN_CHECK_ARG(step_first >= 0 && step_count >= 1 && step_count <= VGAN_AE_MAX_LAUNCH_STEPS && ld_loss >= step_first + step_count);
    VGAN_CHECK_ARG(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0 && weight_decay >= 0.0);
    const long floats = svdd_act_floats(net, max_dims, batch, true);
    const bool lds = floats <= VGAN_AE_LDS_FLOATS;
    VGAN_CHECK_ARG(lds || (scratch && scratch_floats >= floats * count));
    SvddTrain a;
    a.X = X, a.ldx = ldx, a.n = n, a.w = feistel_half_bits((unsigned long long)n), a.feat = feat, a.feat_off = feat_off;
    a.mean = mean, a.scale = scale, a.skip = skip, a.first = first, a.max_dims = max_dims, a.batch = batch, a.spe = n / batch;
    a.seed = seed, a.step_first = step_first, a.step_count = step_count, a.corr = corr;
    a.adam.b1 = (float)beta1, a.adam.omb1 = (float)(1.0 - beta1), a.adam.b2 = (float)beta2, a.adam.omb2 = (float)(1.0 - beta2);
    a.adam.eps = (float)eps, a.adam.wd = (float)weight_decay, a.adam.lr = lr;
    a.center = center, a.state = state, a.s_off = s_off, a.loss = loss, a.ld_loss = ld_loss, a.scratch = scratch, a.scratch_stride = floats;
    const hipStream_t st = (hipStream_t)stream;
    if (lds) {
        static const int allowed = ae_allow_lds(&svdd_train_kernel<true>, __FILE__, __LINE__);
        if (allowed != VGAN_OK) return allowed;
        hipLaunchKernelGGL(svdd_train_kernel<true>, dim3((unsigned)count), dim3(kAeBlock), (size_t)floats * sizeof(float), st, a, net);
    } else {
        hipLaunchKernelGGL(svdd_train_kernel<false>, dim3((unsigned)count), dim3(kAeBlock), 0, st, a, net);
    }
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_svdd_scores(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                                const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                                const int32_t* hidden, int activation, const float* state, const int64_t* s_off, const float* center,
                                float* score, int64_t ld_score, float* embed, float* scratch, int64_t scratch_floats,
                                vgan_stream_t stream) {
    SvddNet net;
    VGAN_CHECK_ARG(X && feat && feat_off && mean && scale && skip && state && s_off && d > 0 && ldx >= d);
    VGAN_CHECK_ARG(rows >= 1 && rows <= VGAN_AE_MAX_ROWS && first >= 0 && count > 0 && count <= 65535 && max_dims >= 1 && max_dims <= VGAN_AE_MAX_DIMS);
    VGAN_CHECK_ARG(svdd_net(n_hidden, hidden, activation, &net));
    VGAN_CHECK_ARG(embed ? count == 1 : (center && score && ld_score >= rows));
    const long floats = svdd_act_floats(net, max_dims, kAeRows, false);
    const long tiles = (rows + kAeRows - 1) / kAeRows;
    VGAN_CHECK_ARG(floats <= VGAN_AE_LDS_FLOATS || (scratch && scratch_floats >= floats * tiles * count));
    SvddScore a;
    a.X = X, a.ldx = ldx, a.rows = rows, a.feat = feat, a.feat_off = feat_off, a.mean = mean, a.scale = scale, a.skip = skip;
    a.first = first, a.max_dims = max_dims, a.state = state, a.s_off = s_off, a.center = center, a.score = score, a.ld_score = ld_score;
    a.embed = embed, a.tsum = nullptr, a.scratch = scratch;
    return svdd_forward_launch(a, net, count, floats, tiles, (hipStream_t)stream);
}

// Deep SVDD one-class scores over the subspaces (Ruff et al. 2018; pyod's DeepSVDD, the one-class objective): one small encoder
// per subspace, trained by Adam on mini-batches to map the standardised rows onto one point c; a row is scored by the squared
// distance of its image from c.  v-gan_amd/outlier.py: SubspaceDeepSVDD, whose docstring is the definition.
// The net, its state, init, the training loop, the scoring forward and the launches are the core of outlier_mlp.hpp (whose
// head comment describes them); this file holds the objective, the centre fold and the entries.  The net has the layer sizes
// K_0 = d_s, h_1 .. h_L (nl = L layers) and NO BIAS anywhere; q = h_L is the output dimension; the target of every row is the
// centre: the error r = out - c, the loss sum r^2 / B, the output error r float32(2 / B).
//
//   centre     the forward of the untrained net over all fitted rows: one workgroup per (block, 32-row tile) sums its outputs
//              per coordinate in float64, rows ascending; a second kernel adds the tile sums to a running float64 sum in tile
//              order and, after the last chunk of rows, divides by n, applies the center_eps rule and rounds to float32.
//   scores     float32(sum_j double(out_j - c_j)^2), j ascending; or the raw output (embed).
#include "outlier_mlp.hpp"

namespace vgan {

constexpr unsigned kSvddPhiloxTag = VGAN_SVDD_PHILOX_TAG;  // "SVD\0" + the layer: counter word 2
constexpr int kSvddFold = VGAN_SVDD_MAX_OUT;               // threads of the fold kernel: one per output coordinate

struct SvddObjective {
    static constexpr bool kBias = false, kMirrored = false, kCenter = true;
    static constexpr int kMaxLayers = VGAN_AE_MAX_HIDDEN;
    __device__ static __forceinline__ int loss_cells(int B, int) { return B; }
    __device__ static __forceinline__ ae_lds_f* center_lds() {
        __shared__ float cs[VGAN_SVDD_MAX_OUT];
        return (ae_lds_f*)cs;
    }
    // z, the outputs of the L layers in a row, the passed-down error: the error of the last layer is its output
    template <class P>
    __device__ static __forceinline__ void place(const MlpNet& net, int ds, int B, P z, int pz, P (&act)[kMaxLayers], int (&pact)[kMaxLayers], P& E,
                                                 int& pe, P& down) {
        const int L = net.nl;
        P at = z + B * pz;
        for (int l = 0; l < kMaxLayers; ++l) {
            if (l < L) {
                act[l] = at, pact[l] = ae_pitch(net.width[l]);
                at += B * pact[l];
            } else {
                act[l] = act[L - 1], pact[l] = pact[L - 1];
            }
        }
        down = at;
        E = act[L - 1], pe = pact[L - 1];
    }
    template <class P>
    __device__ static __forceinline__ float target(int, int o, P, int, ae_lds_f* cs) {
        return cs[o];
    }
    // the output stays in `out`, behind the hidden layers
    template <class P>
    __device__ static __forceinline__ void last_layer(const MlpScore&, P in, int pin, int K, const float* Wl, int q, int B, int, P, int, P out) {
        const int pout = ae_pitch(q);
        ae_forward<false, P>(in, pin, K, Wl, q, B, [&](int i, int o, float val) { out[i * pout + o] = val; });
    }
    template <class P>
    __device__ static __forceinline__ void finish(const MlpScore& a, int B, int row0, P, int, P out, int q, double* tsum) {
        const int tid = threadIdx.x, pout = ae_pitch(q);
        if (a.raw) {
            float* R = a.raw + (long)row0 * q;
            for (int idx = tid; idx < B * q; idx += kAeBlock) {
                const int i = idx / q, o = idx - i * q;
                R[(long)i * q + o] = out[i * pout + o];
            }
        } else if (tsum) {
            if (tid < q) {
                double sum = 0.0;
                for (int i = 0; i < B; ++i) sum += (double)out[i * pout + tid];
                tsum[tid] = sum;
            }
        } else if (tid < B) {
            const float* c = a.center + (long)blockIdx.y * q;
            P orow = out + tid * pout;
            double sum = 0.0;
            for (int f = 0; f < q; ++f) {
                const double d = (double)(orow[f] - c[f]);
                sum += d * d;  // the square of a float32 is exact in float64
            }
            a.score[(long)blockIdx.y * a.ld_score + row0 + tid] = (float)sum;
        }
    }
};

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

extern "C" int vgan_svdd_init(const int32_t* feat_off, int first, int count, int n_hidden, const int32_t* hidden, const double* scale,
                              uint64_t seed, float* state, const int64_t* s_off, int64_t total, vgan_stream_t stream) {
    return mlp_init<SvddObjective>(MLP_HERE, feat_off, first, count, n_hidden, hidden, scale, seed, kSvddPhiloxTag, state, s_off, total, stream);
}

extern "C" int vgan_svdd_center(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                                const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                                const int32_t* hidden, int activation, const float* state, const int64_t* s_off, double* tile_sums,
                                int64_t tile_cells, double* run_sums, int64_t n_total, double center_eps, float* center,
                                int32_t* n_clamped, float* scratch, int64_t scratch_floats, vgan_stream_t stream) {
    MlpScore a;
    MlpNet net;
    long tiles;
    VGAN_CHECK_ARG(tile_sums && run_sums);
    int rc = mlp_forward_args<SvddObjective>(MLP_HERE, X, ldx, rows, d, feat, feat_off, mean, scale, skip, first, count, max_dims, n_hidden,
                                             hidden, activation, state, s_off, scratch, scratch_floats, &a, &net, &tiles);
    if (rc != VGAN_OK) return rc;
    VGAN_CHECK_ARG(n_total >= 0 && n_total <= VGAN_AE_MAX_ROWS && center_eps >= 0.0 && (n_total == 0 || (center && n_clamped)));
    const int q = net.width[net.nl - 1];
    VGAN_CHECK_ARG(tile_cells >= tiles * count * q);
    a.tsum = tile_sums;
    const hipStream_t st = (hipStream_t)stream;
    rc = mlp_forward_launch<SvddObjective>(MLP_HERE, a, net, count, tiles, st);
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
    VGAN_CHECK_ARG(center);
    return mlp_train<SvddObjective>(MLP_HERE, X, ldx, n, d, feat, feat_off, mean, scale, skip, first, count, max_dims, n_hidden, hidden, activation,
                                    batch, seed, step_first, step_count, corr, lr, beta1, beta2, eps, weight_decay, center, state, s_off, loss,
                                    ld_loss, scratch, scratch_floats, stream);
}

extern "C" int vgan_svdd_scores(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                                const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                                const int32_t* hidden, int activation, const float* state, const int64_t* s_off, const float* center,
                                float* score, int64_t ld_score, float* embed, float* scratch, int64_t scratch_floats,
                                vgan_stream_t stream) {
    MlpScore a;
    MlpNet net;
    long tiles;
    const int rc = mlp_forward_args<SvddObjective>(MLP_HERE, X, ldx, rows, d, feat, feat_off, mean, scale, skip, first, count, max_dims, n_hidden,
                                                   hidden, activation, state, s_off, scratch, scratch_floats, &a, &net, &tiles);
    if (rc != VGAN_OK) return rc;
    VGAN_CHECK_ARG(embed ? count == 1 : (center && score && ld_score >= rows));
    a.center = center, a.score = score, a.ld_score = ld_score, a.raw = embed;
    return mlp_forward_launch<SvddObjective>(MLP_HERE, a, net, count, tiles, (hipStream_t)stream);
}

// Autoencoder outlier scores over the subspaces (pyod's AutoEncoder up to dropout and batch normalisation): one small MLP per
// subspace, trained by Adam on mini-batches to reconstruct the standardised rows through a bottleneck; a row is scored by the
// Euclidean norm of its reconstruction error.  v-gan_amd/outlier.py: SubspaceAutoEncoder, whose docstring is the definition.
// The net, its state, init, the training loop, the scoring forward and the launches are the core of outlier_mlp.hpp (whose
// head comment describes them); this file holds the autoencoder's objective and its entries.  The net has the layer sizes K_0 =
// d_s, h_1 .. h_L, h_{L-1} .. h_1, d_s (nl = 2 L layers) and a bias in every layer; the target of a row is the row itself: the
// error r = out - z, the loss sum r^2 / (B d_s), the output error r float32(2 / (B d_s)); the score sqrt(sum_f double(r_f)^2),
// features ascending, or the raw output (reconstruct).
#include "outlier_mlp.hpp"

namespace vgan {

constexpr unsigned kAePhiloxTag = 0x41450000u;  // "AE\0\0" + the layer: counter word 2

struct AeObjective {
    static constexpr bool kBias = true, kMirrored = true, kCenter = false;
    static constexpr int kMaxLayers = 2 * VGAN_AE_MAX_HIDDEN;
    __device__ static __forceinline__ int loss_cells(int B, int ds) { return B * ds; }
    __device__ static __forceinline__ ae_lds_f* center_lds() { return nullptr; }
    // z, E, the hidden layers, the passed-down error: the last layer writes its output into E
    template <class P>
    __device__ static __forceinline__ void place(const MlpNet& net, int ds, int B, P z, int pz, P (&act)[kMaxLayers], int (&pact)[kMaxLayers], P& E,
                                                 int& pe, P& down) {
        E = z + B * pz, pe = pz;
        P at = E + B * pz;
        for (int l = 0; l + 1 < net.nl; ++l) {
            act[l] = at, pact[l] = ae_pitch(net.width[l]);
            at += B * pact[l];
        }
        act[net.nl - 1] = E, pact[net.nl - 1] = pz;
        for (int l = net.nl; l < kMaxLayers; ++l) act[l] = E, pact[l] = pz;
        down = act[net.nl - 2] + B * pact[net.nl - 2];
    }
    template <class P>
    __device__ static __forceinline__ float target(int i, int o, P z, int pz, ae_lds_f*) {
        return z[i * pz + o];
    }
    // the raw output goes to a.raw; else z has been read by layer 0 only and the error takes its place
    template <class P>
    __device__ static __forceinline__ void last_layer(const MlpScore& a, P in, int pin, int K, const float* Wl, int ds, int B, int row0, P z,
                                                      int pz, P) {
        if (a.raw) {
            float* R = a.raw + (long)row0 * ds;
            ae_forward<true, P>(in, pin, K, Wl, ds, B, [&](int i, int o, float val) { R[(long)i * ds + o] = val; });
        } else {
            ae_forward<true, P>(in, pin, K, Wl, ds, B, [&](int i, int o, float val) { z[i * pz + o] = val - z[i * pz + o]; });
        }
    }
    template <class P>
    __device__ static __forceinline__ void finish(const MlpScore& a, int B, int row0, P z, int pz, P, int ds, double*) {
        const int tid = threadIdx.x;
        if (!a.raw && tid < B) {
            P er = z + tid * pz;
            double sum = 0.0;
            for (int f = 0; f < ds; ++f) {
                const double d = (double)er[f];
                sum += d * d;  // the square of a float32 is exact in float64
            }
            a.score[(long)blockIdx.y * a.ld_score + row0 + tid] = (float)sqrt(sum);
        }
    }
};

}  // namespace vgan

using namespace vgan;

extern "C" int vgan_ae_init(const int32_t* feat_off, int first, int count, int n_hidden, const int32_t* hidden, const double* scale,
                            uint64_t seed, float* state, const int64_t* s_off, int64_t total, vgan_stream_t stream) {
    return mlp_init<AeObjective>(MLP_HERE, feat_off, first, count, n_hidden, hidden, scale, seed, kAePhiloxTag, state, s_off, total, stream);
}

extern "C" int vgan_ae_train(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                             const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                             const int32_t* hidden, int activation, int batch, uint64_t seed, int64_t step_first, int step_count,
                             const double* corr, double lr, double beta1, double beta2, double eps, double weight_decay, float* state,
                             const int64_t* s_off, float* loss, int64_t ld_loss, float* scratch, int64_t scratch_floats,
                             vgan_stream_t stream) {
    return mlp_train<AeObjective>(MLP_HERE, X, ldx, n, d, feat, feat_off, mean, scale, skip, first, count, max_dims, n_hidden, hidden, activation,
                                  batch, seed, step_first, step_count, corr, lr, beta1, beta2, eps, weight_decay, nullptr, state, s_off, loss,
                                  ld_loss, scratch, scratch_floats, stream);
}

extern "C" int vgan_ae_scores(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                              const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                              const int32_t* hidden, int activation, const float* state, const int64_t* s_off, float* score,
                              int64_t ld_score, float* recon, float* scratch, int64_t scratch_floats, vgan_stream_t stream) {
    MlpScore a;
    MlpNet net;
    long tiles;
    const int rc = mlp_forward_args<AeObjective>(MLP_HERE, X, ldx, rows, d, feat, feat_off, mean, scale, skip, first, count, max_dims, n_hidden,
                                                 hidden, activation, state, s_off, scratch, scratch_floats, &a, &net, &tiles);
    if (rc != VGAN_OK) return rc;
    VGAN_CHECK_ARG(recon ? count == 1 : (score && ld_score >= rows));
    a.score = score, a.ld_score = ld_score, a.raw = recon;
    return mlp_forward_launch<AeObjective>(MLP_HERE, a, net, count, tiles, (hipStream_t)stream);
}

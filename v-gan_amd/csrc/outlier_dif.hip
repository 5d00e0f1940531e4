// Deep isolation forest (Xu, Pang, Wang, Wang, TKDE 2023; pyod's DIF) over the subspaces, first half: an ensemble of randomly
// initialised, never trained MLPs maps the rows of every subspace to small representations; the isolation trees grown on them
// are those of outlier_iforest.hip (vgan_iforest_build_blocks / vgan_iforest_path_sums_blocks).  Block b = s r + j is
// representation j of subspace s; its net has the layer sizes K_0 = d_s, the hidden widths, q, no bias, and the activation
// after every layer but the last.
//
//   weights    W_l[o, i] of block b from the Philox4x32-10 words of counter (e >> 2, 0, 0x44494600 + l, 0), e = o K_l + i, key
//              (lo32(seed) ^ lo32(b), hi32(seed) ^ hi32(b) ^ 0x5bd1e995): word e & 3 is w, u = (w + 0.5) 2^-32 in float64, W =
//              float32((2 u - 1) c_l), c_l = 1 / sqrt(K_l) from the host.  One Philox call per 4 weights.  Layout of a block:
//              layer after layer, W_l QUAD-MAJOR as [ld_l / 4][K_{l+1}][4] with ld_l = K_l rounded up to 8 and ZEROS in the pad
//              positions: W_l[o, i] sits at ((i >> 2) K_{l+1} + o) 4 + (i & 3).  The forward reads 16-byte k-quads, the 32
//              lanes of a half wave those of 32 neighbouring output rows: 512 contiguous bytes, every byte of every cache
//              line used by the instruction that fetches it (row-major rows gave 32 lines of which 32 bytes each were used,
//              and the rest had left the 32 KiB L1 before the next k-groups came for it), and there is no K tail.
//   represent  one workgroup per (block, tile of kDifRows = 32 rows), 4 waves.  Layer 0 stages z = (x - lo) / (hi - lo) of the
//              subspace's features, kDifKTile = 64 at a time, straight from X through the feature list into one of two LDS
//              images (global loads of tile t + 1 are in flight under the MFMAs of tile t; one barrier per tile).  Every
//              later layer reads the whole activation tile [32][width] of the previous one from LDS and writes its own to the
//              other of two activation buffers (layer 2 reuses the buffer of layer 0): nothing goes to global memory between
//              the layers.  A wave owns the 32-column output tiles wave, wave + 4, ... (at most 4: widths <= 512) and keeps
//              one 32x32 accumulator each; the weights are the B operand, read as 16-byte quads from global memory (each
//              workgroup reads a layer once, the workgroups of a block share it through L2).
//   values     an element of R is ONE chain of v_mfma_f32_32x32x2_f32 over k in an order that depends on k alone (k-groups of
//              8 ascending; inside a group the two lane halves interleave): it depends on its row, its block and its column
//              only -- not on the row tile, the launch, or which other blocks share it.  No split-K.
#include "optim_common.hpp"
#include "vgan_common.hpp"

namespace vgan {

constexpr int kDifRows = VGAN_DIF_ROW_TILE;
constexpr int kDifKTile = VGAN_DIF_K_TILE;
constexpr int kDifMaxWidth = VGAN_DIF_MAX_WIDTH;
constexpr int kDifMaxLayers = VGAN_DIF_MAX_HIDDEN + 1;
constexpr int kDifStagePitch = kDifKTile + 4;                 // floats; 4 * odd: conflict-free 16-byte row reads
constexpr int kDifStageFloats = 2 * kDifRows * kDifStagePitch;
constexpr int kDifAheadQuads = 8;                             // weight quads a lane keeps in flight ahead of the MFMAs
constexpr unsigned kDifPhiloxTag = 0x44494600u;               // "DIF\0" + the layer: counter word 2

typedef __attribute__((address_space(3))) float dif_lds_f;
typedef __attribute__((address_space(3))) f32x4 dif_lds_f4;

struct DifNet {
    int nl;                     // layers: hidden + 1
    int width[kDifMaxLayers];   // outputs of layer l; width[nl - 1] = q
    int act;                    // VGAN_DIF_ACT_*
    int r;                      // representations per subspace
};

__host__ __device__ inline int dif_round8(int v) { return (v + 7) & ~7; }
__host__ __device__ inline int dif_pitch(int width) { return ((width + 31) & ~31) + 4; }

__global__ __launch_bounds__(kBlock) void dif_weights_kernel(const int32_t* __restrict__ feat_off, DifNet net, int first,
                                                             const double* __restrict__ scale, unsigned long long seed,
                                                             float* __restrict__ W, const int64_t* __restrict__ w_off) {
    const unsigned long long b = (unsigned long long)first + blockIdx.y;
    const int s = (int)(b / (unsigned)net.r);
    const unsigned k0 = (unsigned)seed ^ (unsigned)b, k1 = (unsigned)(seed >> 32) ^ (unsigned)(b >> 32) ^ 0x5bd1e995u;
    float* out = W + w_off[blockIdx.y];
    int K = feat_off[s + 1] - feat_off[s];
    for (int l = 0; l < net.nl; ++l) {
        const int N = net.width[l], ld = dif_round8(K);
        const long total = (long)N * K;
        const double c = scale[(long)s * net.nl + l];
        for (long g = (long)blockIdx.x * kBlock + threadIdx.x; 4 * g < total; g += (long)gridDim.x * kBlock) {
            unsigned ctr[4] = {(unsigned)g, (unsigned)((unsigned long long)g >> 32), kDifPhiloxTag + (unsigned)l, 0u};
            philox4x32_10(ctr, k0, k1);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const long e = 4 * g + w;
                if (e < total) {
                    const double u = ((double)ctr[w] + 0.5) * 0x1p-32;  // exact
                    const long o = e / K, i = e % K;
                    out[((i >> 2) * N + o) * 4 + (i & 3)] = (float)((2.0 * u - 1.0) * c);
                }
            }
        }
        out += (long)N * ld;
        K = N;
    }
}

// acc[j] += A[32 rows][8 groups .. ] . W_j^T over `groups` k-groups of 8 starting at k-group g0 of the LDS image and at column
// wk of the weights; lane (fi, fh) feeds row fi of A and output column fi of each of its tiles; wrow[j] points at quad 0 of the
// lane's output row, and quad t of it lies t * quad floats further on
template <int NT>
__device__ __forceinline__ void dif_mma(const dif_lds_f* img, int pitch, int g0, int groups, const float* (&wrow)[NT > 0 ? NT : 1],
                                        bool (&live)[NT > 0 ? NT : 1], int wk, long quad, f32x16 (&acc)[NT > 0 ? NT : 1], int fi, int fh) {
    if constexpr (NT > 0) {
        const dif_lds_f* ap = img + fi * pitch + 8 * g0 + 4 * fh;
        // the weight quads of kDifAhead k-groups are in flight under the MFMAs of the current one (a ring of registers; the
        // loads past the last group repeat it and are not used): the order of the chain stays c ascending.  A wave with one
        // tile has 4 MFMAs (256 cycles) a group to hide a load under, so it looks 8 groups ahead; one with 4 tiles two.
        constexpr int kDifAhead = kDifAheadQuads / NT;
        float4 ring[kDifAhead][NT];
#pragma unroll
        for (int p = 0; p < kDifAhead; ++p)
#pragma unroll
            for (int j = 0; j < NT; ++j) ring[p][j] = *reinterpret_cast<const float4*>(wrow[j] + (wk / 4 + 2 * min(p, groups - 1) + fh) * quad);
        auto step = [&](int c, int p, bool refill) {
            const f32x4 a = *(const dif_lds_f4*)(ap + 8 * c);
            float4 bq[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                bq[j] = live[j] ? ring[p][j] : make_float4(0.f, 0.f, 0.f, 0.f);  // a column past the layer's width stays 0
                if (refill) ring[p][j] = *reinterpret_cast<const float4*>(wrow[j] + (wk / 4 + 2 * min(c + kDifAhead, groups - 1) + fh) * quad);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], bq[j].x, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], bq[j].y, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], bq[j].z, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], bq[j].w, acc[j], 0, 0, 0);
            }
        };
        // whole rounds of the ring run without a branch, so that the wait before a group counts the loads issued after its
        // own and leaves them in flight; the groups left over are in the ring already
        const int whole = groups / kDifAhead * kDifAhead;
        for (int c0 = 0; c0 < whole; c0 += kDifAhead) {
#pragma unroll
            for (int p = 0; p < kDifAhead; ++p) step(c0 + p, p, true);
        }
#pragma unroll
        for (int p = 0; p < kDifAhead - 1; ++p)
            if (whole + p < groups) step(whole + p, p, false);
    }
}

__device__ __forceinline__ float dif_activate(float a, int act) {
    return act == VGAN_DIF_ACT_RELU ? fmaxf(a, 0.f) : (float)tanh((double)a);
}

// What every layer shares.  FIRST: the A operand is z of the subspace, staged from X; otherwise the LDS image `in`.
struct DifTile {
    const float* X;
    long ldx;
    int rows, row0;
    const int32_t* feat;
    const float *lo, *hi;
    int ds;
    dif_lds_f* stage;
};

template <int NT, bool FIRST>
__device__ __forceinline__ void dif_layer(const DifTile& t, const dif_lds_f* in, int pitch_in, int K, const float* __restrict__ Wl, int N,
                                          bool last, int act, dif_lds_f* out, int pitch_out, float* __restrict__ Rb, int q) {
    constexpr int NA = NT > 0 ? NT : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 31, fh = lane >> 5;
    const int ld = dif_round8(K);
    const float* wrow[NA];
    bool live[NA];
    f32x16 acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int o = (wave + 4 * j) * 32 + fi;
        live[j] = o < N;
        wrow[j] = Wl + (long)min(o, N - 1) * 4;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    }
    if constexpr (FIRST) {
        // thread -> feature k0 + (tid & 63) of the rows (tid >> 6) + 4 e: unconditional loads from clamped addresses
        constexpr int PER = kDifRows / (kBlock / kDifKTile);
        const int kk = tid & (kDifKTile - 1), rr = tid >> 6;
        float x[PER];
        float flo = 0.f, fhi = 0.f;
        bool in_k = false;
        auto load = [&](int k0) {
            const int k = k0 + kk;
            in_k = k < t.ds;
            const long col = t.feat[min(k, t.ds - 1)];
            flo = t.lo[col];
            fhi = t.hi[col];
#pragma unroll
            for (int e = 0; e < PER; ++e) x[e] = t.X[(long)min(t.row0 + rr + 4 * e, t.rows - 1) * t.ldx + col];
        };
        auto store = [&](dif_lds_f* img) {
            const double dlo = (double)flo, den = (double)fhi - dlo;
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const float z = (in_k && fhi != flo) ? (float)(((double)x[e] - dlo) / den) : 0.f;
                img[(rr + 4 * e) * kDifStagePitch + kk] = z;
            }
        };
        const int nk = (K + kDifKTile - 1) / kDifKTile;
        load(0);
        for (int kt = 0; kt < nk; ++kt) {
            dif_lds_f* img = t.stage + (kt & 1) * (kDifRows * kDifStagePitch);
            store(img);
            __syncthreads();  // image kt is whole; everybody is done with image kt - 1, which iteration kt + 1 refills
            if (kt + 1 < nk) load((kt + 1) * kDifKTile);
            dif_mma<NT>(img, kDifStagePitch, 0, min(kDifKTile, ld - kt * kDifKTile) / 8, wrow, live, kt * kDifKTile, 4L * N, acc, fi, fh);
        }
    } else {
        dif_mma<NT>(in, pitch_in, 0, ld / 8, wrow, live, 0, 4L * N, acc, fi, fh);
    }
    if constexpr (NT > 0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = (wave + 4 * j) * 32 + fi;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (last) {
                    if (t.row0 + row < t.rows && col < q) Rb[(long)(t.row0 + row) * q + col] = acc[j][r];
                } else {
                    out[row * pitch_out + col] = dif_activate(acc[j][r], act);  // columns N .. round32(N) - 1 receive act(0) = 0
                }
            }
        }
    }
}

template <bool FIRST>
__device__ __forceinline__ void dif_layer_any(int nt, const DifTile& t, const dif_lds_f* in, int pitch_in, int K, const float* __restrict__ Wl,
                                              int N, bool last, int act, dif_lds_f* out, int pitch_out, float* __restrict__ Rb, int q) {
    switch (nt) {  // the tiles of this wave: the same for all of its lanes
        case 0: dif_layer<0, FIRST>(t, in, pitch_in, K, Wl, N, last, act, out, pitch_out, Rb, q); break;
        case 1: dif_layer<1, FIRST>(t, in, pitch_in, K, Wl, N, last, act, out, pitch_out, Rb, q); break;
        case 2: dif_layer<2, FIRST>(t, in, pitch_in, K, Wl, N, last, act, out, pitch_out, Rb, q); break;
        case 3: dif_layer<3, FIRST>(t, in, pitch_in, K, Wl, N, last, act, out, pitch_out, Rb, q); break;
        default: dif_layer<4, FIRST>(t, in, pitch_in, K, Wl, N, last, act, out, pitch_out, Rb, q); break;
    }
}

__global__ __launch_bounds__(kBlock) void dif_represent_kernel(const float* __restrict__ X, long ldx, int rows, const int32_t* __restrict__ feat,
                                                               const int32_t* __restrict__ feat_off, const float* __restrict__ lo,
                                                               const float* __restrict__ hi, DifNet net, int first,
                                                               const float* __restrict__ W, const int64_t* __restrict__ w_off,
                                                               float* __restrict__ R, int pitch_a, int pitch_b) {
    extern __shared__ __attribute__((aligned(16))) float dif_lds_generic[];
    dif_lds_f* lds = (dif_lds_f*)dif_lds_generic;
    dif_lds_f* buf[2] = {lds + kDifStageFloats, lds + kDifStageFloats + kDifRows * pitch_a};
    const int pitch[2] = {pitch_a, pitch_b};
    const int wave = threadIdx.x >> 6;
    const int s = (first + (int)blockIdx.y) / net.r;
    const int off = feat_off[s];
    DifTile t;
    t.X = X, t.ldx = ldx, t.rows = rows, t.row0 = (int)blockIdx.x * kDifRows;
    t.feat = feat + off, t.lo = lo, t.hi = hi, t.ds = feat_off[s + 1] - off, t.stage = lds;
    const float* Wl = W + w_off[blockIdx.y];
    float* Rb = R + (long)blockIdx.y * rows * net.width[net.nl - 1];
    const int q = net.width[net.nl - 1];
    int K = t.ds;
    for (int l = 0; l < net.nl; ++l) {
        const int N = net.width[l];
        const int tiles = (N + 31) / 32, nt = tiles > wave ? (tiles - wave + 3) / 4 : 0;
        const bool last = l == net.nl - 1;
        dif_lds_f* out = buf[l & 1];
        if (l == 0) {
            dif_layer_any<true>(nt, t, nullptr, 0, K, Wl, N, last, net.act, out, pitch[l & 1], Rb, q);
        } else {
            __syncthreads();  // the activations of layer l - 1 are whole
            dif_layer_any<false>(nt, t, buf[(l - 1) & 1], pitch[(l - 1) & 1], K, Wl, N, last, net.act, out, pitch[l & 1], Rb, q);
        }
        Wl += (long)N * dif_round8(K);
        K = N;
    }
}

}  // namespace vgan

using namespace vgan;

// the net of the arguments; false when a size is out of range
static bool dif_net(int r, int n_hidden, const int32_t* hidden, int q, int activation, DifNet* net) {
    if (r < 1 || r > VGAN_DIF_MAX_NETS || n_hidden < 0 || n_hidden > VGAN_DIF_MAX_HIDDEN || (n_hidden > 0 && !hidden)) return false;
    if (q < 1 || q > VGAN_DIF_MAX_OUT || (activation != VGAN_DIF_ACT_TANH && activation != VGAN_DIF_ACT_RELU)) return false;
    net->nl = n_hidden + 1;
    for (int l = 0; l < n_hidden; ++l) {
        if (hidden[l] < 1 || hidden[l] > kDifMaxWidth) return false;
        net->width[l] = hidden[l];
    }
    net->width[n_hidden] = q;
    for (int l = n_hidden + 1; l < kDifMaxLayers; ++l) net->width[l] = 0;
    net->act = activation;
    net->r = r;
    return true;
}

extern "C" int vgan_dif_weights(const int32_t* feat_off, int r, int first, int count, int n_hidden, const int32_t* hidden, int q,
                                const double* scale, uint64_t seed, float* W, const int64_t* w_off, int64_t total, vgan_stream_t stream) {
    DifNet net;
    VGAN_CHECK_ARG(feat_off && scale && W && w_off && first >= 0 && count > 0 && count <= 65535 && total > 0);
    VGAN_CHECK_ARG(dif_net(r, n_hidden, hidden, q, VGAN_DIF_ACT_TANH, &net) && aligned16(W));
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(W, 0, (size_t)total * sizeof(float), st) != hipSuccess) {  // the pad columns
        set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        (void)hipGetLastError();
        return VGAN_ERR_HIP;
    }
    hipLaunchKernelGGL(dif_weights_kernel, dim3(64, (unsigned)count), dim3(kBlock), 0, st, feat_off, net, first, scale,
                       (unsigned long long)seed, W, w_off);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

extern "C" int vgan_dif_represent(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const float* lo,
                                  const float* hi, int r, int first, int count, int n_hidden, const int32_t* hidden, int q, int activation,
                                  const float* W, const int64_t* w_off, float* R, vgan_stream_t stream) {
    DifNet net;
    VGAN_CHECK_ARG(X && feat && feat_off && lo && hi && W && w_off && R && d > 0 && ldx >= d && rows >= 1 && rows <= VGAN_DIF_MAX_ROWS);
    VGAN_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && dif_net(r, n_hidden, hidden, q, activation, &net) && aligned16(W));
    const int pitch_a = n_hidden >= 1 ? dif_pitch(n_hidden >= 3 ? (hidden[0] > hidden[2] ? hidden[0] : hidden[2]) : hidden[0]) : 0;
    const int pitch_b = n_hidden >= 2 ? dif_pitch(hidden[1]) : 0;
    const int bytes = (kDifStageFloats + kDifRows * (pitch_a + pitch_b)) * (int)sizeof(float);
    constexpr int kMost = (kDifStageFloats + 2 * kDifRows * (kDifMaxWidth + 4)) * (int)sizeof(float);
    static_assert(kMost <= 160 * 1024, "the two activation tiles and the staging images fit the LDS of a CU");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&dif_represent_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kMost);
    if (attr != hipSuccess) {
        set_error("%s:%d: hipFuncSetAttribute failed: %s", __FILE__, __LINE__, hipGetErrorString(attr));
        return VGAN_ERR_HIP;
    }
    hipLaunchKernelGGL(dif_represent_kernel, dim3((unsigned)((rows + kDifRows - 1) / kDifRows), (unsigned)count), dim3(kBlock), bytes,
                       (hipStream_t)stream, X, (long)ldx, rows, feat, feat_off, lo, hi, net, first, W, w_off, R, pitch_a, pitch_b);
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

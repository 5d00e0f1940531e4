// What the detectors on the refined neighbour lists of outlier.hip share (outlier_abod.hip, outlier_cof.hip): the gather of a
// query row's k <= 32 listed reference rows over the features of a subspace, the T x T pair blocks formed from them, and the fill
// of the degenerate rows of a score matrix.  What is summed per pair and what is done with the sums is the detector's.
//
// One wave owns one item (subspace s, query row q), a workgroup four query rows of one subspace (all four waves walk the same
// d_s, so the block barriers are uniform).
//   list     the reference row of every neighbour slot, -1 for a missing neighbour: a slot past k, or an index outside the
//            reference set.  Its placement is the one compile-time trait on which the two detectors differ, Pairs::kListInLds:
//            true   in LDS ([KP] ints per wave, KP = 8 T the padded k) with one `valid` bit per slot a lane stages: no registers
//                   across the feature loop.  COF, whose k <= 32 kernel spills with the list in registers
//            false  in registers, the rows of this lane's own slots (k / 2 ints at W = 32).  ABOD: its accumulators leave the
//                   room, and the LDS form measured 5 to 14 % slower on its launch (profiles/neighbor_core_ab_runs.txt)
//   gather   F_s is walked in blocks of kNbrFB = 32 features.  The k x 32 elements of a block are spread over the lanes
//            feature-fastest (lane -> feature lane % W, neighbour lane / W + (64 / W) t; W = 32, or the next power of two
//            >= d_s in a narrower subspace), so the lanes of a load read neighbouring features of one reference row and a
//            2-feature subspace still fills the wave with 32 neighbours.  The loads of block i + 1 are issued before the
//            pair step of block i and land in registers
//   stage    Pairs::stage(r, q) of the raw float32 values goes to LDS as float64, feature-major ([32][KP + 2] per wave; the pad
//            of one 16-byte access keeps the rows off a power-of-two stride).  The slot of a missing neighbour holds exactly 0.
//            With Pairs::kQueryInPad the query's value of the feature sits in the first pad slot (index KP), the 33rd point at no
//            re-tiling
//   pairs    lane (I, J) = (lane / 8, lane % 8) owns the T x T block of pairs (T I + i, T J + j) (T = 1, 2, 4 for k <= 8, 16,
//            32): per feature, in ascending order, it reads 2 T doubles from LDS (one or two 16-byte reads per operand, every
//            address shared by eight lanes) and hands them to Pairs::update with the feature's row.  The whole matrix is
//            formed, not the upper triangle: the lanes below the diagonal would idle otherwise, their cost is the same wave
//            instruction
// A Pairs policy:
//   static constexpr bool kQueryInPad, kListInLds;
//   static double stage(float r, float q);                                  the staged value of a present neighbour
//   void update(const double* row, const double (&av)[T], const double (&bv)[T]);   row[a]: neighbour a, row[KP]: the query
#pragma once
#include <math.h>

#include <type_traits>

#include "vgan_common.hpp"

namespace vgan {

constexpr int kNbrFB = 32;                  // features per staged block
constexpr int kNbrWaves = kBlock / kWave;   // items (query rows) per workgroup

struct NbrArgs {
    const float* Xq;
    int ldq, nq;
    const float* Xr;
    int ldr, nr;
    const int32_t* feat;
    const int32_t* feat_off;
    int first;
    const int32_t* idx;
    int k;
};

template <int T>
struct NbrItem {
    static constexpr int KP = 8 * T, LD = KP + 2;
    int z, q, lane, wave, I, J;
    int q_raw;    // >= nq on a surplus wave: it repeats the last row as q (barriers stay uniform) and stores nothing
    double* V;    // the wave's staging buffer [kNbrFB][LD], free once the last barrier of the caller's own has passed
};

template <int T, class Pairs>
__device__ __forceinline__ NbrItem<T> nbr_pair_blocks(const NbrArgs& g, Pairs& pairs) {
    constexpr int KP = NbrItem<T>::KP, LD = NbrItem<T>::LD;
    constexpr int NE = KP * kNbrFB / kWave;  // staged elements per lane and feature block
    __shared__ __attribute__((aligned(16))) double lds_v[kNbrWaves][kNbrFB * LD];
    __shared__ int lds_nb[kNbrWaves][KP];  // not allocated unless Pairs::kListInLds

    const int k = g.k, z = blockIdx.y, s = g.first + z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q_raw = blockIdx.x * kNbrWaves + wave;
    const int q = min(q_raw, g.nq - 1);
    const int f0 = g.feat_off[s], ds = g.feat_off[s + 1] - f0;
    double* V = lds_v[wave];

    // lanes over (neighbour, feature), feature fastest: W features side by side, 64 / W neighbours per load
    int logw = 5;
    while (logw > 0 && (1 << (logw - 1)) >= ds) --logw;
    const int W = 1 << logw, c = lane & (W - 1), a0 = lane >> logw, astep = kWave >> logw;

    const int32_t* list = g.idx + ((long)z * g.nq + q) * k;
    const auto listed = [&](int a) {
        const int r = a < k ? list[a] : -1;
        return (unsigned)r < (unsigned)g.nr ? r : -1;
    };
    int nb[Pairs::kListInLds ? 1 : NE];
    unsigned valid = 0;
    if constexpr (Pairs::kListInLds) {
        if (lane < KP) lds_nb[wave][lane] = listed(lane);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int a = a0 + t * astep;
            if (a < KP && lds_nb[wave][a] >= 0) valid |= 1u << t;
        }
    } else {
#pragma unroll
        for (int t = 0; t < NE; ++t) nb[t] = listed(a0 + t * astep);
    }
    const auto row_of = [&](int t) {  // the reference row of slot t, a valid one for a missing neighbour too
        if constexpr (Pairs::kListInLds) return max(lds_nb[wave][min(a0 + t * astep, KP - 1)], 0);
        else return max(nb[t], 0);
    };
    const float* xq = g.Xq + (long)q * g.ldq;

    // every load is unconditional inside a wave-uniform guard (slots past k are skipped by the whole wave); a lane past
    // d_s or on a missing neighbour reads a valid address again and its value is dropped when the block is staged
    float qv = 0.f, rv[NE];
    bool live = false;
#pragma unroll
    for (int t = 0; t < NE; ++t) rv[t] = 0.f;
    auto load_block = [&](int cb) {
        live = cb + c < ds;
        const int f = g.feat[f0 + min(cb + c, ds - 1)];
        qv = xq[f];
#pragma unroll
        for (int t = 0; t < NE; ++t)
            if (t * astep < k) rv[t] = g.Xr[(long)row_of(t) * g.ldr + f];
    };

    const int I = lane >> 3, J = lane & 7;
    load_block(0);
    for (int cb = 0; cb < ds; cb += kNbrFB) {
        __syncthreads();  // the pair step of the previous block has read its LDS
        // `valid` is made opaque here: left loop-invariant, its 16 bit tests are hoisted as 16 lane masks and spill SGPRs.
        // A slot past KP (narrow subspaces only) has no bit and writes its 0 to the unused second pad slot; with the list in
        // registers such a slot is skipped
        if constexpr (Pairs::kListInLds) asm volatile("" : "+v"(valid));
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int a = a0 + t * astep;
            if constexpr (Pairs::kListInLds)
                V[c * LD + min(a, KP) + (a >= KP ? 1 : 0)] = (live && (valid >> t & 1u)) ? Pairs::stage(rv[t], qv) : 0.0;
            else if (a < KP)
                V[c * LD + a] = (live && nb[t] >= 0) ? Pairs::stage(rv[t], qv) : 0.0;
        }
        if (Pairs::kQueryInPad && a0 == 0) V[c * LD + KP] = live ? (double)qv : 0.0;
        __syncthreads();
        if (cb + kNbrFB < ds) load_block(cb + kNbrFB);
        const int cw = min(kNbrFB, ds - cb);
        for (int f = 0; f < cw; ++f) {
            const double* row = V + f * LD;
            double av[T], bv[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                av[i] = row[T * I + i];
                bv[i] = row[T * J + i];
            }
            pairs.update(row, av, bv);
        }
    }
    return {z, q, lane, wave, I, J, q_raw, V};
}

// launch(std::integral_constant<int, T>) with the pair-block edge T of k: launch(t) names its kernel as kernel<decltype(t)::value>
template <class Launch>
inline void dispatch_nbr_tile(int k, Launch&& launch) {
    if (k <= 8)
        launch(std::integral_constant<int, 1>{});
    else if (k <= 16)
        launch(std::integral_constant<int, 2>{});
    else
        launch(std::integral_constant<int, 4>{});
}

inline dim3 nbr_grid(int nq, int count) { return dim3((nq + kNbrWaves - 1) / kNbrWaves, count); }

// One workgroup per row s of the score matrix [S, ld] (n scores a row).  A NaN score marks a degenerate row.  kMax: the fill
// value is the row's largest score that is not NaN, 1 if there is none; otherwise its smallest, 0 if there is none.
//   fit != 0  value[s] = that fill value, n_degenerate[s] = the number of NaNs
//   then every NaN of the row becomes (float)value[s].  An extreme and an integer count are order-free.
template <bool kMax>
__global__ __launch_bounds__(kBlock) void fill_degenerate_kernel(float* __restrict__ score, int ld, int n, int fit,
                                                                 double* __restrict__ value, int32_t* __restrict__ n_degenerate) {
    __shared__ float red_m[kBlock / kWave];
    __shared__ int red_c[kBlock / kWave];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto extreme = [](float a, float b) { return kMax ? fmaxf(a, b) : fminf(a, b); };
    float* row = score + (long)s * ld;
    float fill;
    if (fit) {
        float m = kMax ? -INFINITY : INFINITY;
        int cnt = 0;
        for (int i = tid; i < n; i += kBlock) {
            const float v = row[i];
            if (v == v) m = extreme(m, v);
            else ++cnt;
        }
        m = kMax ? wave_max(m) : wave_min(m);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            red_m[wave] = m;
            red_c[wave] = cnt;
        }
        __syncthreads();
        m = extreme(extreme(red_m[0], red_m[1]), extreme(red_m[2], red_m[3]));
        cnt = red_c[0] + red_c[1] + red_c[2] + red_c[3];
        fill = cnt == n ? (kMax ? 1.f : 0.f) : m;
        if (tid == 0) {
            value[s] = (double)fill;
            n_degenerate[s] = cnt;
        }
    } else {
        fill = (float)value[s];
    }
    for (int i = tid; i < n; i += kBlock) {
        const float v = row[i];
        if (!(v == v)) row[i] = fill;
    }
}

template <bool kMax>
inline void launch_fill_degenerate(float* score, int ld, int S, int n, int fit, double* value, int32_t* n_degenerate,
                                   vgan_stream_t stream) {
    hipLaunchKernelGGL(fill_degenerate_kernel<kMax>, dim3(S), dim3(kBlock), 0, (hipStream_t)stream, score, ld, n, fit ? 1 : 0, value,
                       n_degenerate);
}

}  // namespace vgan

// Shared device/host helpers for the V-GAN gfx950 kernels (CDNA4: 64-wide waves, fp32 MFMA).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vgan_hip.h"

namespace vgan {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;
constexpr int kBlock = 256;  // 4 waves, one per SIMD; two such workgroups per CU hide epilogues

void set_error(const char* fmt, ...);

// The _AT forms report a given file and line: a routine shared by several entries names the entry that called it.  The
// condition is turned into text where it is written, before its macros expand.
#define VGAN_CHECK_ARG_TEXT(file, line, cond, text)                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            ::vgan::set_error("%s:%d: bad argument: %s", (file), (line), text);    \
            return VGAN_ERR_ARG;                                                   \
        }                                                                          \
    } while (0)
#define VGAN_CHECK_ARG(cond) VGAN_CHECK_ARG_TEXT(__FILE__, __LINE__, cond, #cond)
#define VGAN_CHECK_ARG_AT(file, line, cond) VGAN_CHECK_ARG_TEXT(file, line, cond, #cond)

#define VGAN_CHECK_LAUNCH_AT(file, line)                                                              \
    do {                                                                                              \
        hipError_t e_ = hipGetLastError();                                                            \
        if (e_ != hipSuccess) {                                                                       \
            ::vgan::set_error("%s:%d: launch failed: %s", (file), (line), hipGetErrorString(e_));     \
            return VGAN_ERR_HIP;                                                                      \
        }                                                                                             \
    } while (0)
#define VGAN_CHECK_LAUNCH() VGAN_CHECK_LAUNCH_AT(__FILE__, __LINE__)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// float64 sum over a kBlock-thread workgroup in a fixed order (wave butterfly, then the four waves in order); red: 4 doubles
// of LDS; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
// the same sum, valid in every thread; red may be written again at once
__device__ __forceinline__ double block_sum_all(double v, double* red) {
    const double r = block_sum(v, red);
    __syncthreads();
    return r;
}

// a * b rounded to float64 before anything is added to it.  The library is built with -ffp-contract=fast, under which a product
// and the sum that takes it become one v_fma_f64, HIP's __dmul_rn / __dadd_rn included (they are plain operators there): the
// empty asm makes the product a value the optimiser cannot look through, so the sum that follows is a second rounding, as
// numpy's and libsvm's is.  It also keeps the compiler from unrolling a loop around it: callers that want that unroll by hand.
__device__ __forceinline__ double mul_rounded(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}
// The same without volatile, for a product between LDS reads (outlier_inne.hip, outlier_sod.hip): the statement has to stay
// opaque, not in place.  A volatile one orders the LDS reads around it, and iNNE's pair loop then waits out one read per
// centre (measured on the MI355X: 1.3 times the time of the scoring pass at d = 784).
__device__ __forceinline__ double mul_rounded_free(double a, double b) {
    double p = a * b;
    asm("" : "+v"(p));
    return p;
}

// Column-max key: U > 0 always, so its IEEE bits order like the value; ties go to the LOWEST row.
__device__ __forceinline__ unsigned long long colkey_pack(float u, unsigned row) {
    return ((unsigned long long)__float_as_uint(u) << 32) | (unsigned long long)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ float colkey_value(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32)); }
__device__ __forceinline__ unsigned colkey_row(unsigned long long k) { return 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull); }

// Column arg-max of U over one chunk of kColChunkRows rows for 64 columns (block bx covers columns 64*bx.., chunk by).
// Shared by the stand-alone kernel (rows.hip) and by the Gram launch, which runs it in surplus workgroups.
constexpr int kColChunkRows = 64;
template <int NW>  // waves in the calling workgroup: ALL of them take part (rows are dealt round-robin over the waves)
__device__ __forceinline__ void colmax_partial_body(const float* __restrict__ S, int lds, int row_offset,
                                                    unsigned long long* __restrict__ part, int n, int d, int from_softmax, int bx,
                                                    int by) {
    __shared__ unsigned long long colmax_red[NW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = bx * 64 + lane;
    const int r0 = by * kColChunkRows;
    const float tau = from_softmax ? 1.0f / (float)d : INFINITY;  // U given directly: no threshold
    unsigned long long best = 0ull;
    if (j < d) {
        // all loads of the chunk are issued before the first compare (the blocks that run this inside the Gram launch are
        // latency-bound); rows past the end are clamped to the last row, whose key they merely repeat
        // (NW need not divide the chunk: a wave's surplus turn repeats the chunk's last row, and a max does not mind)
        constexpr int PER = (kColChunkRows + NW - 1) / NW;
        float sv[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) sv[e] = S[(long)min(r0 + min(wave + e * NW, kColChunkRows - 1), n - 1) * lds + j];
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const unsigned long long k = colkey_pack(sv[e] < tau ? sv[e] : 1.0f,
                                                     (unsigned)(row_offset + min(r0 + min(wave + e * NW, kColChunkRows - 1), n - 1)));
            best = k > best ? k : best;
        }
    }
    colmax_red[wave][lane] = best;
    __syncthreads();
    if (wave == 0 && j < d) {
        unsigned long long b = colmax_red[0][lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) b = colmax_red[w][lane] > b ? colmax_red[w][lane] : b;
        part[(long)by * d + j] = b;
    }
}

// z = hi + lo with hi = bf16(z) (round to nearest even), lo = bf16(z - hi): the operand split of the bf16x3 MMD kernels
__device__ __forceinline__ unsigned short bf16_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }
__device__ __forceinline__ float bf16_val(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
__device__ __forceinline__ void split_bf16(float v, unsigned short& hi, unsigned short& lo) {
    hi = bf16_bits(v);
    lo = bf16_bits(v - bf16_val(hi));
}

// the value the split operands carry: hi + lo (16 significant bits of v); row norms of the bf16x3 kernels are taken from it
__device__ __forceinline__ float split_value(float v) {
    unsigned short hi, lo;
    split_bf16(v, hi, lo);
    return bf16_val(hi) + bf16_val(lo);
}

// ---- one element of the centred MMD operand Z = [X - c ; U * X - c] and of the multiplier X, from x, u and the centre c ------
// Two launches form these numbers independently -- the mask / projection launch that writes the operand, and the 64-wide
// split-bf16 MMD backward when it rebuilds its epilogue operands instead of reading an fp32 copy of Z -- and they must agree
// bit for bit, so every operation is spelled out here instead of being left to -ffp-contract:
//   centred_x          fl(x - c)            one subtraction;
//   project_centred    fma(u, x, -c)        ONE rounding.  The reference rounds the product `U * batch` (src/vgan.py:616) before
//                      any distance is taken, and this function used to ask for that with `#pragma clang fp contract(off)` --
//                      but the library is built with -ffp-contract=fast, under which the back end fuses across the pragma: the
//                      object code has always held v_fma_f32 / v_pk_fma_f32 here (read off the disassembly), and every recorded
//                      result was computed with it.  It is written as what it is; the difference to the reference's form is
//                      half an ulp of u * x, below the split-bf16 operand's own resolution;
//   uncentred_x        fl(xc + c)           the batch entry as the backward's multiplier sees it: mul + mul_shift.
__device__ __forceinline__ float centred_x(float x, float c) { return __fsub_rn(x, c); }
__device__ __forceinline__ float project_centred(float u, float x, float c) { return __fmaf_rn(u, x, -c); }
__device__ __forceinline__ float uncentred_x(float xc, float c) { return __fadd_rn(xc, c); }
// the mask entry of a softmax value (src/models/Generator.py:20-21), tau = float32(1 / d)
__device__ __forceinline__ float upper_mask(float s, float tau) { return s < tau ? s : 1.0f; }

// ---- counter-based random permutation of [0, N): balanced Feistel network + cycle walking ---------------------------
// A 2w-bit balanced Feistel network (2^(2w) >= N, < 4N) with a keyed 32-bit mixer as round function is a bijection of
// [0, 2^(2w)) for ANY round function; walking the cycle until the value drops below N restricts it to a bijection of [0, N)
// (expected < 4 evaluations).  Every index is computed independently: 16 B of state, no table, no sort, no atomics.
__host__ __device__ inline unsigned feistel_mix(unsigned x, unsigned k) {
    x ^= k;
    x *= 0x9E3779B1u;
    x ^= x >> 15;
    x *= 0x85EBCA77u;
    x ^= x >> 13;
    x *= 0xC2B2AE3Du;
    x ^= x >> 16;
    return x;
}
constexpr int kFeistelRounds = 8;
__host__ __device__ inline unsigned long long feistel_perm(unsigned long long i, unsigned long long N, int w, unsigned long long seed,
                                                           unsigned long long epoch) {
    const unsigned mask = (w >= 32) ? 0xFFFFFFFFu : ((1u << w) - 1u);
    const unsigned k0 = (unsigned)seed ^ 0xA511E9B3u, k1 = (unsigned)(seed >> 32) ^ (unsigned)epoch, k2 = (unsigned)(epoch >> 32) ^ 0x63D83595u;
    unsigned long long v = i;
    do {
        unsigned l = (unsigned)(v >> w) & mask, r = (unsigned)v & mask;
#pragma unroll
        for (int q = 0; q < kFeistelRounds; ++q) {
            const unsigned f = feistel_mix(r, feistel_mix(k0 + 0x9E3779B9u * (unsigned)q, k1) ^ k2) & mask;
            const unsigned nl = r;
            r = l ^ f;
            l = nl;
        }
        v = ((unsigned long long)l << w) | r;
    } while (v >= N);
    return v;
}

// w of feistel_perm for a range of N values: the smallest w <= 32 with 2^(2w) >= N
inline int feistel_half_bits(unsigned long long N) {
    int w = 1;
    while (w < 32 && (1ull << (2 * w)) < N) ++w;
    return w;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace vgan

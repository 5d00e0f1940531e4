// Grouped small-GEMM launch: up to four independent row-major products in ONE launch.
//
// The collapsed generator (src/models/Generator.py:61-66 has no activation between its Linear layers) is a chain of
// small matrix products; each launch of a dependent chain costs ~5 us whatever its size, so products that do not depend
// on each other share a launch.  Per problem the library picks the tile engine: 32x32 tiles with K split over the waves
// (GemmTileKS) when the 64x64 grid would be a handful of long-K tiles, 64x64x32 tiles otherwise.
#include "gemm_core.hpp"
#include "mmd_common.hpp"
#include "optim_common.hpp"

namespace vgan {

constexpr int QBM = 64, QBK = 32, QKS = 128;

struct GroupedArgs {
    vgan_gemm_problem p[VGAN_GEMM_MAX_GROUP];
    int tile_start[VGAN_GEMM_MAX_GROUP + 1];
    int ks[VGAN_GEMM_MAX_GROUP];
    int split[VGAN_GEMM_MAX_GROUP];   // K slices of the problem (vgan_gemm_problem.splitk): slice s writes slab s of C
    int kchunk[VGAN_GEMM_MAX_GROUP];  // contraction indices per slice (a multiple of QBK)
    int count;
};

// One K slice of a split problem as a problem of its own: operands advanced along the contraction, output = slab `slice`.
__device__ __forceinline__ vgan_gemm_problem k_slice(vgan_gemm_problem q, int slice, int kchunk) {
    const int k0 = slice * kchunk;
    q.c += (long)slice * q.m * q.ldc;
    if (q.kind == VGAN_GEMM_NN) { q.a += k0; q.b += (long)k0 * q.ldb; }
    else if (q.kind == VGAN_GEMM_NT) { q.a += k0; q.b += k0; }
    else { q.a += (long)k0 * q.lda; q.b += (long)k0 * q.ldb; }
    q.k = min(kchunk, q.k - k0);
    return q;
}

// What may ride in a grouped launch besides its products (vgan_gemm_grouped_ex): a plain copy, the Adadelta update as
// the products' epilogue (+ one element-wise layer whose gradient already sits in memory), and the next step's noise draw.
struct GroupedExtras {
    const float* copy_src;
    float* copy_dst;
    long copy_count;
    int copy_blocks, extra_blocks, noise_blocks, adadelta;
    float *p, *sq, *acc;
    float lr, rho, eps, wd, gs;
    vgan_adadelta_layer layer[VGAN_GEMM_MAX_GROUP + 1];
    const float* g_extra;
    int ld_extra;
    float* z;
    int zrows, zcols, zld, zones;
    unsigned long long seed;
    const unsigned long long* step_counter;
    int fold_blocks;
    vgan_finalize_job fold;
};

// the optimiser step of one element of a packed gradient image [dW | db]: (row, col) -> flat parameter index
__device__ __forceinline__ void adadelta_packed_element(const GroupedExtras& x, const vgan_adadelta_layer& L, int row, int col, float g) {
    if (row >= L.out || col > L.in) return;
    const long idx = col < L.in ? L.off_w + (long)row * L.in + col : L.off_b + row;
    float pv = x.p[idx], v = x.sq[idx], a = x.acc[idx];
    adadelta_one(pv, g, v, a, x.lr, x.rho, x.eps, x.wd, x.gs);
    x.p[idx] = pv;
    x.sq[idx] = v;
    x.acc[idx] = a;
    L.w_packed[(long)row * L.ldp + col] = pv;
}

// The same for the NE elements a lane holds of an output tile (one column, NE rows), in two phases: the optimiser state is
// REQUESTED before the product's main loop (it does not depend on the product; requested after it the launch pays one more
// memory latency per tile -- measured 11.5 us for the launch instead of the product's ~6) and ALL loads precede the first store
// (the pointers may alias as far as the compiler knows: element-by-element code serialises NE round trips, 16.2 us).
template <int NE>
struct AdadeltaTile {
    long idx[NE];
    float pv[NE], v[NE], a[NE];
    bool ok[NE];
    template <typename RowOf>
    __device__ __forceinline__ void prefetch(const GroupedExtras& x, const vgan_adadelta_layer& L, int col, RowOf row_of) {
#pragma unroll
        for (int r = 0; r < NE; ++r) {
            const int row = row_of(r);
            ok[r] = row < L.out && col <= L.in;
            idx[r] = ok[r] ? (col < L.in ? L.off_w + (long)row * L.in + col : L.off_b + row) : L.off_w;  // clamped: unconditional loads
            pv[r] = x.p[idx[r]];
            v[r] = x.sq[idx[r]];
            a[r] = x.acc[idx[r]];
        }
    }
    template <typename RowOf>
    __device__ __forceinline__ void finish(const GroupedExtras& x, const vgan_adadelta_layer& L, int col, const float (&g)[NE], RowOf row_of) {
#pragma unroll
        for (int r = 0; r < NE; ++r) adadelta_one(pv[r], g[r], v[r], a[r], x.lr, x.rho, x.eps, x.wd, x.gs);
#pragma unroll
        for (int r = 0; r < NE; ++r)
            if (ok[r]) {
                x.p[idx[r]] = pv[r];
                x.sq[idx[r]] = v[r];
                x.acc[idx[r]] = a[r];
                L.w_packed[(long)row_of(r) * L.ldp + col] = pv[r];
            }
    }
};

// workgroups past the product tiles: copy | element-wise layer | noise (block-uniform dispatch)
__device__ __forceinline__ void grouped_extra_jobs(const GroupedExtras& x, int b, int layer_index) {
    if (b < x.copy_blocks) {
        for (long i = (long)b * blockDim.x + threadIdx.x; i < x.copy_count; i += (long)x.copy_blocks * blockDim.x) x.copy_dst[i] = x.copy_src[i];
        return;
    }
    b -= x.copy_blocks;
    if (b < x.extra_blocks) {
        const vgan_adadelta_layer& L = x.layer[layer_index];
        const long total = (long)L.out * (L.in + 1);
        for (long i = (long)b * blockDim.x + threadIdx.x; i < total; i += (long)x.extra_blocks * blockDim.x) {
            const int row = (int)(i / (L.in + 1)), col = (int)(i % (L.in + 1));
            adadelta_packed_element(x, L, row, col, x.g_extra[(long)row * x.ld_extra + col]);
        }
        return;
    }
    b -= x.extra_blocks;
    if (b < x.noise_blocks) {
        noise_normal_body(x.z, x.zrows, x.zcols, x.zld, x.zones, x.seed, x.step_counter, 0ull, b, x.noise_blocks);
        return;
    }
    b -= x.noise_blocks;
    if (b < x.fold_blocks) finalize_body(x.fold);
}

template <int LA, int LB, int VEC, bool EPI>
__device__ __forceinline__ void tile64(const vgan_gemm_problem& q, int t, float* lds, const GroupedExtras& x, int qi) {
    using G = GemmTile<QBM, QBM, QBK, LA, LB, VEC>;
    const int gx = (q.n + QBM - 1) / QBM;
    const int m0 = (t / gx) * QBM, n0 = (t % gx) * QBM;
    const int col = n0 + G::sub_col(0);
    auto row_of = [&](int r) { return m0 + G::sub_row(0, r); };
    AdadeltaTile<EPI ? 16 : 1> upd;
    if constexpr (EPI) upd.prefetch(x, x.layer[qi], col, row_of);
    f32x16 acc[1][1];
    zero_acc(acc);
    G::template run<false>(q.a, q.lda, q.b, q.ldb, m0, n0, q.m, q.n, q.k, lds, nullptr, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + G::sub_row(0, r);
        if (row < q.m && col < q.n) q.c[(long)row * q.ldc + col] = acc[0][0][r];
    }
    if constexpr (EPI) {
        float g[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = acc[0][0][r];
        upd.finish(x, x.layer[qi], col, g, row_of);
    }
}

template <int LA, int LB, int VEC, int NW = 4, bool EPI = false>
__device__ __forceinline__ void tile_ks(const vgan_gemm_problem& q, int t, float* lds, const GroupedExtras& x, int qi) {
    using G = GemmTileKS<QKS, LA, LB, VEC, NW>;
    const int gx = (q.n + 31) / 32;
    const int m0 = (t / gx) * 32, n0 = (t % gx) * 32;
    const int col = n0 + G::col_of();
    auto row_of = [&](int rr) { return m0 + G::row_of(rr); };
    AdadeltaTile<EPI ? G::NR : 1> upd;
    if constexpr (EPI) upd.prefetch(x, x.layer[qi], col, row_of);
    float o[G::NR];
    G::run(q.a, q.lda, q.b, q.ldb, m0, n0, q.m, q.n, q.k, lds, o);
#pragma unroll
    for (int rr = 0; rr < G::NR; ++rr) {
        const int row = m0 + G::row_of(rr);
        if (row < q.m && col < q.n) q.c[(long)row * q.ldc + col] = o[rr];
    }
    if constexpr (EPI) upd.finish(x, x.layer[qi], col, o, row_of);
}

// C tile = (A[m0 .., :k] . B[:k2, :k]^T) . D[n0 .., :k2]^T: the tile's 64 rows of H = A . B^T go through the problem's scratch
// region (global memory, L2-hot: written and re-read by this workgroup only, behind a __syncthreads, whose fence drains the
// stores), then the second product reads them as its A operand.
template <int VEC>
__device__ __forceinline__ void tile64_two_stage(const vgan_gemm_problem& q, int t, float* lds) {
    using G = GemmTile<QBM, QBM, QBK, KC, KC, VEC>;
    const int gx = (q.n + QBM - 1) / QBM;
    const int m0 = (t / gx) * QBM, n0 = (t % gx) * QBM;
    const int ldh = (q.k2 + 3) / 4 * 4;
    float* H = q.scratch + (long)t * QBM * ldh;
    const int rows = min(QBM, q.m - m0);
    for (int c0 = 0; c0 < q.k2; c0 += QBM) {
        f32x16 acc[1][1];
        zero_acc(acc);
        G::template run<false>(q.a, q.lda, q.b, q.ldb, m0, c0, q.m, q.k2, q.k, lds, nullptr, acc);
        const int col = c0 + G::sub_col(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = G::sub_row(0, r);
            if (row < rows && col < ldh) H[(long)row * ldh + col] = col < q.k2 ? acc[0][0][r] : 0.f;
        }
    }
    __syncthreads();
    f32x16 acc[1][1];
    zero_acc(acc);
    G::template run<false>(H, ldh, q.d, q.ldd, 0, n0, rows, q.n, q.k2, lds, nullptr, acc);
    const int col = n0 + G::sub_col(0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + G::sub_row(0, r);
        if (row < q.m && col < q.n) q.c[(long)row * q.ldc + col] = acc[0][0][r];
    }
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int VEC, bool EPI>
__global__ __launch_bounds__(kBlock, 2) void gemm_grouped_kernel(GroupedArgs g, GroupedExtras x) {
    constexpr int kLds = cmax(cmax(GemmTile<QBM, QBM, QBK, KC, MC, VEC>::kLdsFloats, GemmTile<QBM, QBM, QBK, MC, MC, VEC>::kLdsFloats),
                              cmax(cmax(GemmTileKS<QKS, KC, MC, VEC>::kLdsFloats, GemmTileKS<QKS, MC, MC, VEC>::kLdsFloats),
                                   cmax(GemmTile<QBM, QBM, QBK, KC, KC, VEC>::kLdsFloats, GemmTileKS<QKS, KC, KC, VEC>::kLdsFloats)));
    __shared__ __attribute__((aligned(16))) float lds[kLds];
    if ((int)blockIdx.x >= g.tile_start[VGAN_GEMM_MAX_GROUP]) {  // block-uniform: the jobs riding behind the product tiles
        grouped_extra_jobs(x, blockIdx.x - g.tile_start[VGAN_GEMM_MAX_GROUP], g.count);
        return;
    }
    int qi = 0;  // block-uniform
#pragma unroll
    for (int i = 1; i < VGAN_GEMM_MAX_GROUP; ++i)
        if (i < g.count && (int)blockIdx.x >= g.tile_start[i]) qi = i;
    vgan_gemm_problem q = g.p[qi];
    int t = blockIdx.x - g.tile_start[qi];
    if (g.split[qi] > 1) {  // (block-uniform) tiles of slice 0, then of slice 1, ...
        const int per = (g.tile_start[qi + 1] - g.tile_start[qi]) / g.split[qi];
        q = k_slice(q, t / per, g.kchunk[qi]);
        t %= per;
    }
    // operand images: KC = contraction index contiguous ([mn][K]), MC = output index contiguous ([K][mn])
    if (q.kind == VGAN_GEMM_NN) {         // C = A[m,k] . B[k,n]
        if (g.ks[qi]) tile_ks<KC, MC, VEC, 4, EPI>(q, t, lds, x, qi); else tile64<KC, MC, VEC, EPI>(q, t, lds, x, qi);
    } else if (q.kind == VGAN_GEMM_NT) {  // C = A[m,k] . B[n,k]^T
        if (g.ks[qi]) tile_ks<KC, KC, VEC, 4, EPI>(q, t, lds, x, qi); else tile64<KC, KC, VEC, EPI>(q, t, lds, x, qi);
    } else if (q.kind == VGAN_GEMM_NT_NT) {  // C = (A[m,k] . B[k2,k]^T) . D[n,k2]^T
        tile64_two_stage<VEC>(q, t, lds);
    } else {                              // C = A[k,m]^T . B[k,n]
        if (g.ks[qi]) tile_ks<MC, MC, VEC, 4, EPI>(q, t, lds, x, qi); else tile64<MC, MC, VEC, EPI>(q, t, lds, x, qi);
    }
}

// Every problem on 32x32 tiles with 16 waves splitting K (1024-thread workgroups): launches whose products all have a long
// contraction, where the per-wave MFMA chain is the critical path.
__global__ __launch_bounds__(1024, 1) void gemm_grouped_ks16_kernel(GroupedArgs g, GroupedExtras x) {
    constexpr int kLds = cmax(cmax(GemmTileKS<QKS, KC, MC, 4, 16>::kLdsFloats, GemmTileKS<QKS, MC, MC, 4, 16>::kLdsFloats),
                              GemmTileKS<QKS, KC, KC, 4, 16>::kLdsFloats);
    __shared__ __attribute__((aligned(16))) float lds[kLds];
    if ((int)blockIdx.x >= g.tile_start[VGAN_GEMM_MAX_GROUP]) {  // (this variant carries the copy job only)
        grouped_extra_jobs(x, blockIdx.x - g.tile_start[VGAN_GEMM_MAX_GROUP], g.count);
        return;
    }
    int qi = 0;
#pragma unroll
    for (int i = 1; i < VGAN_GEMM_MAX_GROUP; ++i)
        if (i < g.count && (int)blockIdx.x >= g.tile_start[i]) qi = i;
    const vgan_gemm_problem& q = g.p[qi];
    const int t = blockIdx.x - g.tile_start[qi];
    if (q.kind == VGAN_GEMM_NN) tile_ks<KC, MC, 4, 16>(q, t, lds, x, qi);
    else if (q.kind == VGAN_GEMM_NT) tile_ks<KC, KC, 4, 16>(q, t, lds, x, qi);
    else tile_ks<MC, MC, 4, 16>(q, t, lds, x, qi);
}

// The same launch with some problems' contraction cut over several workgroups per tile and combined in the launch
// (ksplit_finish, gemm_core.hpp).  A problem's workgroups are its tiles of part 0, then of part 1, ...
struct GroupedKSplit {
    KSplitWs ws;
    int parts[VGAN_GEMM_MAX_GROUP], kchunk[VGAN_GEMM_MAX_GROUP];
    int slot0[VGAN_GEMM_MAX_GROUP];  // first ticket of the problem
    int slab0[VGAN_GEMM_MAX_GROUP];  // byte offset of its first slab
};

template <int LA, int LB>
__device__ __forceinline__ void tile_ks_split(const vgan_gemm_problem& q, int t, int part, int parts, int kchunk, const KSplitWs& ws, int slot,
                                              int slab0, float* lds) {
    using G = GemmTileKS<QKS, LA, LB, 4, 16>;
    const int gx = (q.n + 31) / 32;
    const int m0 = (t / gx) * 32, n0 = (t % gx) * 32;
    const int k0 = part * kchunk, klen = min(kchunk, q.k - k0);
    float o[G::NR];
    if (klen > 0) {  // (block-uniform)
        const float* a = q.a + (LA == KC ? (long)k0 : (long)k0 * q.lda);
        const float* b = q.b + (LB == KC ? (long)k0 : (long)k0 * q.ldb);
        G::run(a, q.lda, b, q.ldb, m0, n0, q.m, q.n, klen, lds, o);
    } else {
#pragma unroll
        for (int rr = 0; rr < G::NR; ++rr) o[rr] = 0.f;
    }
    if (!ksplit_finish<G::NR, G::NTH>(o, ws, slot, slab0, part, parts, lds)) return;
    const int col = n0 + G::col_of();
#pragma unroll
    for (int rr = 0; rr < G::NR; ++rr) {
        const int row = m0 + G::row_of(rr);
        if (row < q.m && col < q.n) q.c[(long)row * q.ldc + col] = o[rr];
    }
}

__global__ __launch_bounds__(1024, 1) void gemm_grouped_ks16_split_kernel(GroupedArgs g, GroupedExtras x, GroupedKSplit ks) {
    constexpr int kLds = cmax(cmax(GemmTileKS<QKS, KC, MC, 4, 16>::kLdsFloats, GemmTileKS<QKS, MC, MC, 4, 16>::kLdsFloats),
                              GemmTileKS<QKS, KC, KC, 4, 16>::kLdsFloats);
    __shared__ __attribute__((aligned(16))) float lds[kLds];
    if ((int)blockIdx.x >= g.tile_start[VGAN_GEMM_MAX_GROUP]) {
        grouped_extra_jobs(x, blockIdx.x - g.tile_start[VGAN_GEMM_MAX_GROUP], g.count);
        return;
    }
    int qi = 0;
#pragma unroll
    for (int i = 1; i < VGAN_GEMM_MAX_GROUP; ++i)
        if (i < g.count && (int)blockIdx.x >= g.tile_start[i]) qi = i;
    const vgan_gemm_problem& q = g.p[qi];
    int t = blockIdx.x - g.tile_start[qi];
    const int parts = ks.parts[qi];
    if (parts <= 1) {  // (block-uniform)
        if (q.kind == VGAN_GEMM_NN) tile_ks<KC, MC, 4, 16>(q, t, lds, x, qi);
        else if (q.kind == VGAN_GEMM_NT) tile_ks<KC, KC, 4, 16>(q, t, lds, x, qi);
        else tile_ks<MC, MC, 4, 16>(q, t, lds, x, qi);
        return;
    }
    const int per = (g.tile_start[qi + 1] - g.tile_start[qi]) / parts;
    const int part = t / per;
    t %= per;
    const int slot = ks.slot0[qi] + t, slab0 = ks.slab0[qi] + t * parts * kKSplitSlabBytes, kc = ks.kchunk[qi];
    if (q.kind == VGAN_GEMM_NN) tile_ks_split<KC, MC>(q, t, part, parts, kc, ks.ws, slot, slab0, lds);
    else if (q.kind == VGAN_GEMM_NT) tile_ks_split<KC, KC>(q, t, part, parts, kc, ks.ws, slot, slab0, lds);
    else tile_ks_split<MC, MC>(q, t, part, parts, kc, ks.ws, slot, slab0, lds);
}

}  // namespace vgan

using namespace vgan;

static inline int extra_grid(long work_items) {
    long g = (work_items + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : (g > 256 ? 256 : g));
}

// tickets and slabs an in-launch K split of these problems needs (0: nothing is split); -1: bad arguments
static int64_t ksplit_need(const vgan_gemm_problem* problems, int count, const int32_t* kparts) {
    if (!problems || count < 1 || count > VGAN_GEMM_MAX_GROUP) return -1;
    long split_tiles = 0, slabs = 0;
    for (int i = 0; i < count; ++i) {
        const int parts = kparts ? kparts[i] : 1;
        if (parts < 1 || parts > kKSplitMaxParts || problems[i].m <= 0 || problems[i].n <= 0) return -1;
        if (parts == 1) continue;
        const long t32 = (long)((problems[i].m + 31) / 32) * ((problems[i].n + 31) / 32);
        split_tiles += t32;
        slabs += t32 * parts;
    }
    return split_tiles == 0 ? 0 : ksplit_ticket_bytes(split_tiles) + slabs * kKSplitSlabBytes;
}

// ---- dispatch: grouped_plan validates the arguments and fills the kernels' argument blocks; its return value names the launch
// (enum vgan_gemm_grouped_path_code) or is < 0 where the entry points return VGAN_ERR_ARG.  It launches nothing and dereferences
// no operand pointer.  grouped_launch switches on that value and the host-side query vgan_gemm_grouped_path returns it, so the
// query and the launch cannot disagree.  check_ws: the in-launch K split's workspace is validated too (the query has none).
#define VGAN_PLAN_CHECK(cond)                                                       \
    do {                                                                            \
        if (!(cond)) {                                                              \
            ::vgan::set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond); \
            return -VGAN_ERR_ARG;                                                   \
        }                                                                           \
    } while (0)

struct GroupedPlan {
    GroupedArgs g{};
    GroupedExtras x{};
    GroupedKSplit ks{};
    int blocks = 0;      // workgroups of the launch, riders included
    int slots = 0;       // tickets of the in-launch K split
    int slab_bytes = 0;  // and its slab region
};

static int grouped_plan(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras, const int32_t* kparts,
                        const void* ws, int64_t ws_bytes, bool check_ws, GroupedPlan& plan) {
    VGAN_PLAN_CHECK(problems && count >= 1 && count <= VGAN_GEMM_MAX_GROUP);
    bool ksplit = false;
    for (int i = 0; i < count && kparts != nullptr; ++i) {
        VGAN_PLAN_CHECK(kparts[i] >= 1 && kparts[i] <= kKSplitMaxParts);
        VGAN_PLAN_CHECK(kparts[i] == 1 || problems[i].splitk <= 1);  // slabs of C for the caller, or the in-launch combine: not both
        ksplit = ksplit || kparts[i] > 1;
    }
    if (ksplit) {
        const int64_t need = ksplit_need(problems, count, kparts);
        VGAN_PLAN_CHECK(need > 0 && need < (1ll << 31));
        if (check_ws) VGAN_PLAN_CHECK(ws != nullptr && aligned16(ws) && ws_bytes >= need);
    }
    GroupedArgs& g = plan.g;
    GroupedExtras& x = plan.x;
    g.count = count;
    bool vec = true, any_split = false;
    int tiles = 0;
    for (int i = 0; i < count; ++i) {
        const vgan_gemm_problem& q = problems[i];
        VGAN_PLAN_CHECK(q.a && q.b && q.c && q.m > 0 && q.n > 0 && q.k > 0 && q.ldc >= q.n);
        VGAN_PLAN_CHECK(q.kind == VGAN_GEMM_NN || q.kind == VGAN_GEMM_NT || q.kind == VGAN_GEMM_TN || q.kind == VGAN_GEMM_NT_NT);
        const bool two = q.kind == VGAN_GEMM_NT_NT;
        VGAN_PLAN_CHECK(q.lda >= (q.kind == VGAN_GEMM_TN ? q.m : q.k) && q.ldb >= ((q.kind == VGAN_GEMM_NT || two) ? q.k : q.n));
        if (two) {
            VGAN_PLAN_CHECK(q.d && q.scratch && q.k2 > 0 && q.ldd >= q.k2 && q.splitk <= 1 && aligned16(q.scratch));
            vec = vec && (q.k2 % 4 == 0) && (q.ldd % 4 == 0) && aligned16(q.d);
            any_split = true;  // (keeps the launch on the 64 x 64 tile kernel, without the optimiser epilogue)
        }
        vec = vec && (q.m % 4 == 0) && (q.n % 4 == 0) && (q.k % 4 == 0) && (q.lda % 4 == 0) && (q.ldb % 4 == 0) && aligned16(q.a) &&
              aligned16(q.b);
        const long t64 = (long)((q.m + 63) / 64) * ((q.n + 63) / 64);
        // a long contraction over few tiles: the K loop is the critical path -> 32x32 tiles with K split over the waves, as
        // long as they still fit the chip in one round (2 workgroups per CU)
        const long t32 = (long)((q.m + 31) / 32) * ((q.n + 31) / 32);
        g.ks[i] = (q.k >= 128 && t32 <= 512 && !two) ? 1 : 0;
        g.p[i] = q;
        g.tile_start[i] = tiles;
        // split-K across WORKGROUPS (splitk > 1): a product with a long contraction and too few 64 x 64 tiles to load the chip
        // evenly (c5: M_3 = Wt_4^T M_4 is 165 tiles of K = 4100) is cut into splitk slices of the contraction; slice s writes
        // its partial product to slab s of C (slabs m * ldc floats apart) and the caller sums them in fixed order
        // (vgan_reduce_slabs) -- no atomics, so replicas of a data-parallel run stay bit-identical.
        g.split[i] = q.splitk > 1 ? q.splitk : 1;
        if (g.split[i] > 1) {
            g.kchunk[i] = ((q.k + g.split[i] - 1) / g.split[i] + QBK - 1) / QBK * QBK;
            VGAN_PLAN_CHECK(g.split[i] <= 64 && (long)(g.split[i] - 1) * g.kchunk[i] < q.k);  // every slice holds work
            g.ks[i] = 0;
            any_split = true;
        }
        tiles += g.ks[i] ? ((q.m + 31) / 32) * ((q.n + 31) / 32) : (int)t64 * g.split[i];
    }
    for (int i = count; i <= VGAN_GEMM_MAX_GROUP; ++i) g.tile_start[i] = tiles;
    bool epi = false;
    if (extras != nullptr) {
        const vgan_grouped_extras& e = *extras;
        if (e.copy_src != nullptr) {
            VGAN_PLAN_CHECK(e.copy_dst && e.copy_count > 0);
            x.copy_src = e.copy_src;
            x.copy_dst = e.copy_dst;
            x.copy_count = (long)e.copy_count;
            x.copy_blocks = extra_grid(e.copy_count);
        }
        if (e.adadelta) {
            VGAN_PLAN_CHECK(e.p && e.sq_avg && e.acc_delta && !any_split);  // (the optimiser epilogue needs the whole product)
            epi = true;
            x.adadelta = 1;
            x.p = e.p; x.sq = e.sq_avg; x.acc = e.acc_delta;
            x.lr = e.lr; x.rho = e.rho; x.eps = e.eps; x.wd = e.weight_decay; x.gs = e.grad_scale;
            const int nl = count + (e.g_extra != nullptr ? 1 : 0);
            for (int i = 0; i < nl; ++i) {
                const vgan_adadelta_layer& L = e.layer[i];
                VGAN_PLAN_CHECK(L.w_packed && L.out > 0 && L.in > 0 && L.ldp >= L.in + 1 && L.off_w >= 0 && L.off_b >= 0);
                if (i < count) VGAN_PLAN_CHECK(problems[i].m >= L.out && problems[i].n >= L.in + 1);
                x.layer[i] = L;
            }
            if (e.g_extra != nullptr) {
                VGAN_PLAN_CHECK(e.ld_extra >= e.layer[count].in + 1);
                x.g_extra = e.g_extra;
                x.ld_extra = e.ld_extra;
                x.extra_blocks = extra_grid((long)e.layer[count].out * (e.layer[count].in + 1));
            }
        }
        if (e.next_noise != nullptr) {
            VGAN_PLAN_CHECK(e.noise_rows > 0 && e.noise_cols > 0 && e.noise_ld >= e.noise_cols && e.noise_ones_col < e.noise_ld);
            x.z = e.next_noise;
            x.zrows = e.noise_rows; x.zcols = e.noise_cols; x.zld = e.noise_ld; x.zones = e.noise_ones_col;
            x.seed = (unsigned long long)e.seed;
            x.step_counter = reinterpret_cast<const unsigned long long*>(e.step_counter);
            x.noise_blocks = extra_grid(((long)e.noise_rows * e.noise_cols + 3) / 4);
        }
        if (e.fold != nullptr) {
            VGAN_PLAN_CHECK(finalize_job_ok(*e.fold));
            x.fold = *e.fold;
            x.fold_blocks = 1;
        }
    }
    const int surplus = x.copy_blocks + x.extra_blocks + x.noise_blocks + x.fold_blocks;
    // all products long-K and few tiles: one 1024-thread launch with every problem on 32x32 tiles (no optimiser epilogue there)
    int kmin = problems[0].k, t32 = 0;
    for (int i = 0; i < count; ++i) {
        kmin = problems[i].k < kmin ? problems[i].k : kmin;
        t32 += ((problems[i].m + 31) / 32) * ((problems[i].n + 31) / 32);
    }
    const bool ks16 = vec && kmin >= 96 && t32 <= 256 && !epi && x.noise_blocks == 0 && !any_split;  // (copy and fold jobs ride in this variant too)
    VGAN_PLAN_CHECK(!ksplit || ks16);  // the in-launch K split exists for the 16-wave launch only
    if (ks16) {
        GroupedKSplit& ks = plan.ks;
        int acc = 0, slots = 0, slab_bytes = 0;
        for (int i = 0; i < count; ++i) {
            const int tiles_i = ((problems[i].m + 31) / 32) * ((problems[i].n + 31) / 32);
            const int parts = ksplit ? kparts[i] : 1;
            g.ks[i] = 1;
            g.tile_start[i] = acc;
            acc += tiles_i * parts;
            ks.parts[i] = parts;
            if (parts > 1) {
                ks.kchunk[i] = ksplit_kchunk(problems[i].k, parts, QKS);
                ks.slot0[i] = slots;
                ks.slab0[i] = slab_bytes;
                slots += tiles_i;
                slab_bytes += tiles_i * parts * kKSplitSlabBytes;
            }
        }
        for (int i = count; i <= VGAN_GEMM_MAX_GROUP; ++i) g.tile_start[i] = acc;
        plan.blocks = acc + surplus;
        plan.slots = slots;
        plan.slab_bytes = slab_bytes;
        return ksplit ? VGAN_GEMM_GROUPED_KS16_SPLIT : VGAN_GEMM_GROUPED_KS16;
    }
    plan.blocks = tiles + surplus;
    if (vec) return epi ? VGAN_GEMM_GROUPED_T256_V4_EPI : VGAN_GEMM_GROUPED_T256_V4;
    return epi ? VGAN_GEMM_GROUPED_T256_V1_EPI : VGAN_GEMM_GROUPED_T256_V1;
}

static int grouped_launch(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras, const int32_t* kparts, void* ws,
                          int64_t ws_bytes, vgan_stream_t stream) {
    GroupedPlan plan;
    const int path = grouped_plan(problems, count, extras, kparts, ws, ws_bytes, true, plan);
    if (path < 0) return VGAN_ERR_ARG;
    const GroupedArgs& g = plan.g;
    const GroupedExtras& x = plan.x;
    const dim3 grid(plan.blocks);
    hipStream_t st = (hipStream_t)stream;
    switch (path) {
        case VGAN_GEMM_GROUPED_KS16_SPLIT:
            plan.ks.ws = KSplitWs{reinterpret_cast<float*>(static_cast<char*>(ws) + ksplit_ticket_bytes(plan.slots)), static_cast<int*>(ws),
                                  plan.slab_bytes};
            hipLaunchKernelGGL(gemm_grouped_ks16_split_kernel, grid, dim3(1024), 0, st, g, x, plan.ks);
            break;
        case VGAN_GEMM_GROUPED_KS16: hipLaunchKernelGGL(gemm_grouped_ks16_kernel, grid, dim3(1024), 0, st, g, x); break;
        case VGAN_GEMM_GROUPED_T256_V4_EPI: hipLaunchKernelGGL((gemm_grouped_kernel<4, true>), grid, dim3(kBlock), 0, st, g, x); break;
        case VGAN_GEMM_GROUPED_T256_V4: hipLaunchKernelGGL((gemm_grouped_kernel<4, false>), grid, dim3(kBlock), 0, st, g, x); break;
        case VGAN_GEMM_GROUPED_T256_V1_EPI: hipLaunchKernelGGL((gemm_grouped_kernel<1, true>), grid, dim3(kBlock), 0, st, g, x); break;
        default: hipLaunchKernelGGL((gemm_grouped_kernel<1, false>), grid, dim3(kBlock), 0, st, g, x); break;  // VGAN_GEMM_GROUPED_T256_V1
    }
    VGAN_CHECK_LAUNCH();
    return VGAN_OK;
}

// per problem: the tile engine (enum vgan_gemm_engine) the launch named by the return value runs it on
extern "C" int vgan_gemm_grouped_path(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras, const int32_t* kparts,
                                      int32_t* engine) {
    GroupedPlan plan;
    const int path = grouped_plan(problems, count, extras, kparts, nullptr, 0, false, plan);
    if (path < 0) return path;
    const bool ks16 = path == VGAN_GEMM_GROUPED_KS16 || path == VGAN_GEMM_GROUPED_KS16_SPLIT;
    for (int i = 0; i < count && engine != nullptr; ++i)
        engine[i] = ks16 ? VGAN_GEMM_ENGINE_KS16 : plan.g.ks[i] ? VGAN_GEMM_ENGINE_KS4 : VGAN_GEMM_ENGINE_T64;
    return path;
}

extern "C" int vgan_gemm_grouped_ex(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras,
                                    vgan_stream_t stream) {
    return grouped_launch(problems, count, extras, nullptr, nullptr, 0, stream);
}

extern "C" int64_t vgan_gemm_grouped_ksplit_ws_bytes(const vgan_gemm_problem* problems, int count, const int32_t* kparts) {
    const int64_t need = ksplit_need(problems, count, kparts);
    return need < 0 ? 0 : need;
}

extern "C" int vgan_gemm_grouped_ksplit(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras,
                                        const int32_t* kparts, void* ws, int64_t ws_bytes, vgan_stream_t stream) {
    return grouped_launch(problems, count, extras, kparts, ws, ws_bytes, stream);
}

extern "C" int vgan_gemm_grouped(const vgan_gemm_problem* problems, int count, vgan_stream_t stream) {
    return vgan_gemm_grouped_ex(problems, count, nullptr, stream);
}

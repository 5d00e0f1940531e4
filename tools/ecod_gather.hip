// Ablation for csrc/outlier_ecod.hip (ECOD): the masked sums of the per-feature terms as a plain
// gather-sum instead of the dense float64 product with the 0/1 mask.  One thread per (subspace, row), lanes along the rows:
// it walks the feature list of its subspace and adds T[row, f] in float64, features ascending, then rounds to float32 --
// the same numbers as aggregate "dimension" of vgan_ecod_scores up to the order inside the matrix unit.  Not part of the
// library; tools/outlier_bench.py --method ecod loads it.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC tools/ecod_gather.hip -o tools/bin/libecod_gather.so
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(256) void ecod_gather_kernel(const double* __restrict__ T, long rows, int d, const int32_t* __restrict__ feat,
                                                          const int32_t* __restrict__ feat_off, float* __restrict__ out, long ld_out) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (r >= rows) return;
    const double* row = T + r * d;
    double acc = 0.0;
    for (int k = feat_off[s]; k < feat_off[s + 1]; ++k) acc += row[feat[k]];
    out[(long)s * ld_out + r] = (float)acc;
}

// T [rows, d] float64 terms, feat / feat_off: the concatenated ascending feature lists of the S subspaces, out [S, ld_out]
extern "C" int ecod_gather_sum(const double* T, long rows, int d, const int32_t* feat, const int32_t* feat_off, int S, float* out,
                               long ld_out, void* stream) {
    if (!T || !feat || !feat_off || !out || rows <= 0 || d <= 0 || S <= 0 || S > 65535 || ld_out < rows) return 1;
    hipLaunchKernelGGL(ecod_gather_kernel, dim3((unsigned)((rows + 255) / 256), S), dim3(256), 0, (hipStream_t)stream, T, rows, d, feat,
                       feat_off, out, ld_out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

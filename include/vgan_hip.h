/*
 * vgan_hip.h -- C ABI of libvgan_hip.so: the MI355X (gfx950) kernels behind the V-GAN training
 * hot path (reference: jcribeiro98/V-GAN, src/vgan.py:597-621 and src/models/ *.py).
 *
 * The reference is pure Python/PyTorch and has no FFI of its own; each entry point below replaces
 * the ATen op sequence of one reference module call, cited as file:line of the reference checkout.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to float32 (unless typed otherwise), row-major, with an
 *     explicit leading dimension (elements);  the caller owns and allocates every buffer,
 *     including workspaces;  the library keeps no state between calls (the frozen RBF bandwidth
 *     lives in a caller-owned device scalar);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never synchronises
 *     the host, never allocates, and is therefore HIP-graph capturable;
 *   - return value: 0 = VGAN_OK, otherwise an error code; vgan_last_error() gives the text.
 */
#ifndef VGAN_HIP_H
#define VGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGAN_OK 0
#define VGAN_ERR_ARG 1  /* bad shape / null pointer / unsupported configuration */
#define VGAN_ERR_HIP 2  /* a HIP runtime call or launch failed */

#define VGAN_ABI_VERSION 11 /* counts layout / signature changes; the *_ksplit, *_path, vgan_ecod_*, vgan_iforest_*, vgan_hist_*, vgan_hbos_*, vgan_loda_*, vgan_inne_*, vgan_sos_*, vgan_dif_*, vgan_sod_*, vgan_kpca_*, vgan_ae_*, vgan_svdd_*, vgan_hics_*, vgan_iforest_*_blocks, vgan_outlier_*_metric, vgan_outlier_pack_unit, vgan_loci_*, vgan_rshash_* and vgan_iforest_*_oblique entry points only ADD symbols, so it stands */

typedef void* vgan_stream_t; /* hipStream_t */

int vgan_abi_version(void);
const char* vgan_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Generator_big / Encoder / Decoder Linear layers  (src/models/Generator.py:61-66,
 * src/models/Detector.py:8-13,24-29: nn.Linear == addmm; autograd: two mm per layer)
 *   W is PyTorch layout [out, in].
 * ------------------------------------------------------------------------------------------- */
/* y[n,out] = x[n,in] . W^T + b            (b may be NULL).
 * x may be given as x_nslabs partial slabs x_slab_stride elements apart (a split-K result that was
 * not reduced yet): they are summed, in ascending order, while the operand is staged. */
int vgan_linear_forward(const float* x, int ldx, int x_nslabs, int64_t x_slab_stride, const float* W,
                        int ldw, const float* b, float* y, int ldy, int n, int in, int out,
                        vgan_stream_t stream);
/* dx[n,in] = dy[n,out] . W */
int vgan_linear_backward_input(const float* dy, int lddy, const float* W, int ldw,
                               float* dx, int lddx, int n, int in, int out, vgan_stream_t stream);
/* dW[out,in] = dy^T . x ;  db[out] = column sums of dy   (db may be NULL).
 * splits > 1: the batch rows are cut into `splits` slices and slice s writes its PARTIAL result to
 * dW + s*slab_stride / db + s*slab_stride (elements); sum the slabs with vgan_reduce_slabs.  The
 * contraction runs over the batch while the outputs are small, so slicing is what fills the chip.
 * A slice is ceil(n / splits) rows rounded up to a multiple of 4; slices past the last row are empty and
 * their slabs (db included) are written as zeros, so the reducer may always sum `splits` slabs.
 * x may itself be given as x_nslabs unreduced slabs (see vgan_linear_forward). */
int vgan_linear_backward_params(const float* dy, int lddy, const float* x, int ldx, int x_nslabs,
                                int64_t x_slab_stride, float* dW, int lddw, float* db, int n, int in,
                                int out, int splits, int64_t slab_stride, vgan_stream_t stream);
/* vgan_linear_backward_params (db == NULL, no slabs) for the training step's M_4 = dlogits^T [z|1] with the X-X tiles of the
 * Gram (struct vgan_xx_job, declared below; identity row map: Dh / Dl / dsq are the step's own Zh / Zl / sq) riding in the
 * launch as surplus workgroups.  Shape contract: the 16-wave tall-skinny kernel's (out, in, leading dimensions % 4 == 0,
 * aligned bases, n >= 256, at most 32 64x64 output tiles). */
struct vgan_xx_job;
int vgan_linear_backward_params_xx_supported(int n, int in, int out); /* host-side query of that contract (1 / 0) */
int vgan_linear_backward_params_xx(const float* dy, int lddy, const float* x, int ldx, float* dW, int lddw, int n, int in,
                                   int out, const struct vgan_xx_job* xx, vgan_stream_t stream);
/* vgan_linear_backward_params (db == NULL, no slabs) on the 16-wave tall-skinny tiles with the contraction of every 32 x 32
 * output tile cut over `parts` workgroups (1..8), part q over the batch rows [q kchunk, (q + 1) kchunk), kchunk = the rows per
 * part rounded up to the 128-deep K tile, and combined INSIDE the launch: every part writes its partial tile to the workspace,
 * the last one to arrive at the tile's ticket sums all parts in part order (deterministic, whoever arrives last), writes dW
 * and resets the ticket.  For a long contraction over so few tiles that most of the chip would idle (the step's M_4: 50 tiles,
 * K = 1024).  parts == 1 IS vgan_linear_backward_params.  parts > 1: the 16-wave kernel's contract (out, in, leading dimensions
 * % 4 == 0, aligned bases) and a 16-byte aligned workspace of at least ..._ws_bytes(in, out, parts) bytes (0 for parts <= 1) that
 * was ZEROED once before its first use and is not shared with a launch that may run at the same time; its first
 * ceil(in/32) * ceil(out/32) int32 words are the tickets, which every launch leaves at 0. */
int64_t vgan_linear_backward_params_ksplit_ws_bytes(int in, int out, int parts);
int vgan_linear_backward_params_ksplit(const float* dy, int lddy, const float* x, int ldx, float* dW, int lddw, int n, int in,
                                       int out, int parts, void* ws, int64_t ws_bytes, vgan_stream_t stream);
/* Host-side path queries (no launch, nothing dereferenced: only nullness and alignment of the pointers are looked at, so they
 * work without a GPU).  Each takes its entry point's arguments without the stream and returns the code of the kernel
 * instantiation that entry point launches for exactly those arguments, or a negative value where it returns VGAN_ERR_ARG.
 * The entry points switch on the same function's value.  T64: 64 x 64 x 32 tiles (GemmTile, 256 threads); KS4 / KS16: 32 x 32
 * tiles with every 128-deep K tile split over 4 / 16 waves (GemmTileKS); V4 / V1: operands staged 16 bytes / one float per
 * lane (V1: some dimension, leading dimension or base address is no multiple of 4 floats); SLABS: the slab-summing stager. */
enum vgan_linear_forward_path_code {
    VGAN_LINEAR_FORWARD_T64_V4 = 0,       /* linear_fwd_kernel<4, false> */
    VGAN_LINEAR_FORWARD_T64_V1 = 1,       /* linear_fwd_kernel<1, false> */
    VGAN_LINEAR_FORWARD_T64_V4_SLABS = 2, /* linear_fwd_kernel<4, true>: x_nslabs > 1 */
    VGAN_LINEAR_FORWARD_T64_V1_SLABS = 3, /* linear_fwd_kernel<1, true> */
    VGAN_LINEAR_FORWARD_KS4_V4 = 4,       /* linear_fwd_ks_kernel<4, 4>: at most 32 64 x 64 tiles, in >= 128 */
    VGAN_LINEAR_FORWARD_KS4_V1 = 5,       /* linear_fwd_ks_kernel<1, 4> */
    VGAN_LINEAR_FORWARD_KS16_V4 = 6,      /* linear_fwd_ks_kernel<4, 16>: the same with in >= 512 */
    VGAN_LINEAR_FORWARD_PATHS = 7
};
enum vgan_linear_backward_input_path_code {
    VGAN_LINEAR_BACKWARD_INPUT_T64_V4 = 0, /* linear_bwd_input_kernel<4> */
    VGAN_LINEAR_BACKWARD_INPUT_T64_V1 = 1, /* linear_bwd_input_kernel<1> */
    VGAN_LINEAR_BACKWARD_INPUT_KS4_V4 = 2, /* linear_bwd_input_ks_kernel<4>: at most 32 64 x 64 tiles, out >= 128; `in` may be ragged
                                            * when ldw >= round4(in): W's columns [in, round4(in)) are then read and never stored */
    VGAN_LINEAR_BACKWARD_INPUT_KS4_V1 = 3, /* linear_bwd_input_ks_kernel<1> */
    VGAN_LINEAR_BACKWARD_INPUT_PATHS = 4
};
enum vgan_linear_backward_params_path_code {
    VGAN_LINEAR_BACKWARD_PARAMS_T64_V4 = 0,       /* linear_bwd_params_kernel<4, false> */
    VGAN_LINEAR_BACKWARD_PARAMS_T64_V1 = 1,       /* linear_bwd_params_kernel<1, false> */
    VGAN_LINEAR_BACKWARD_PARAMS_T64_V4_SLABS = 2, /* linear_bwd_params_kernel<4, true>: x_nslabs > 1 */
    VGAN_LINEAR_BACKWARD_PARAMS_T64_V1_SLABS = 3, /* linear_bwd_params_kernel<1, true> */
    VGAN_LINEAR_BACKWARD_PARAMS_KS4_V4 = 4,       /* linear_bwd_params_ks_kernel<4, 4>: db NULL, no slabs, n >= 128 over few tiles */
    VGAN_LINEAR_BACKWARD_PARAMS_KS4_V1 = 5,       /* linear_bwd_params_ks_kernel<1, 4> */
    VGAN_LINEAR_BACKWARD_PARAMS_KS16_V4 = 6,      /* linear_bwd_params_ks_kernel<4, 16>: the same with n >= 256 */
    VGAN_LINEAR_BACKWARD_PARAMS_PATHS = 7
};
int vgan_linear_forward_path(const float* x, int ldx, int x_nslabs, int64_t x_slab_stride, const float* W, int ldw,
                             const float* b, const float* y, int ldy, int n, int in, int out);
int vgan_linear_backward_input_path(const float* dy, int lddy, const float* W, int ldw, const float* dx, int lddx, int n,
                                    int in, int out);
int vgan_linear_backward_params_path(const float* dy, int lddy, const float* x, int ldx, int x_nslabs, int64_t x_slab_stride,
                                     const float* dW, int lddw, const float* db, int n, int in, int out, int splits,
                                     int64_t slab_stride);
/* dst[i] = sum over s < nslabs of src[s*slab_stride + i], in ascending s (bitwise reproducible) */
int vgan_reduce_slabs(const float* src, int64_t slab_stride, int nslabs, float* dst, int64_t count,
                      vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * upper_softmax + projection  (src/models/Generator.py:18-22, src/vgan.py:616 `U * batch`)
 *   logits [n,d] -> S = softmax rows, U = (S < 1/d ? S : 1), and the two halves of the stacked
 *   MMD operand Z = [X_batch ; U * X_batch]:  Zx[i] = X_batch[i], Zy[i] = U[i] * X_batch[i]
 *   (row stride ldz; columns d..ldz-1 are not written: pre-zero them to pad the feature dimension)
 *   with squared row norms sqx[n], sqy[n].  S, U are dense [n,d].  Zx/sqx may be NULL.
 *   The shuffled-batch gather of the DataLoader (src/vgan.py:578-584, :599) is fused in:
 *   X_batch row i = data[ rows[(t % row_batches) * row_stride + row_offset + i] ], where `rows` is a
 *   whole epoch's table of shuffled indices and t = *row_cursor is the device-side step counter
 *   (row_cursor == NULL: t = 0;  rows == NULL: X_batch row i = data[row_offset + i]).  U may be NULL.
 *   center (may be NULL): a per-feature constant c[d] subtracted from EVERY row of Z, i.e. Zx[i] = X[i] - c and
 *   Zy[i] = fma(U[i], X[i], -c) (one rounding: the library is built with -ffp-contract=fast).  cdist(Z,Z)**2 (Mmd_loss_constrained.py:25) is translation invariant, so the loss and
 *   its gradient are unchanged in exact arithmetic, while a common offset of a feature no longer eats the mantissa of
 *   the fp32 (and above all the split-bf16) operands; the step engine passes the data-set mean (vgan_col_mean).
 *   norm_split != 0: sqx/sqy are the norms of the split values hi + lo that vgan_mmd_bf3_prepare will produce from
 *   Zx/Zy (what vgan_mmd_gram_bf3 needs: L = s_i + s_j - 2 g is then |zhat_i - zhat_j|^2 exactly).
 *   chain (may be NULL): Generator_big collapsed into one matrix (vgan_homogeneous_pack / vgan_gemm_grouped): the launch
 *   computes logits = za . At4^T itself (za [n, ldza] = [z | 1 | 0-pad], At4 [d, ldat], e0 = round4(L + 1) columns used), one
 *   wave per batch row, and `logits` is neither read nor written (may be NULL).  Needs the row-in-registers path: d % 4 == 0,
 *   d <= 1024, aligned bases.  Removes the logits launch and 2 x n d x 4 bytes of traffic from the step.
 * ------------------------------------------------------------------------------------------- */
typedef struct vgan_logits_chain {
    const float* za;
    const float* At4;
    int32_t ldza, ldat, e0, pad;
} vgan_logits_chain;
int vgan_mask_project_forward(const float* logits, int ldl, const float* data, int ldd,
                              const int32_t* rows, const uint64_t* row_cursor, int row_batches,
                              int row_stride, int row_offset, float* S, float* U, float* Zx, float* Zy,
                              int ldz, float* sqx, float* sqy, int n, int d, const float* center,
                              int norm_split, const vgan_logits_chain* chain, vgan_stream_t stream);
/* out[j] = mean over the rows of data[:, j] (float64 accumulation, fixed order): the `center` of the calls above. */
int vgan_col_mean(const float* data, int ldd, int rows, int d, float* out, vgan_stream_t stream);
/* out[i, :d] = data[rows[i], :d], sq[i] = |out[i]|^2 (sq may be NULL): batch rows a rank needs as
 * Gram columns but holds no mask for (data-parallel runs keep the data set replicated). */
int vgan_gather_rows(const float* data, int ldd, const int32_t* rows, const uint64_t* row_cursor,
                     int row_batches, int row_stride, int row_offset, float* out, int ldo,
                     float* sq, int n, int d, vgan_stream_t stream);
/* The X half of the (centred) MMD operand alone, for a batch whose mask does not exist yet: out[i] = data[rows[i]] - center
 * (out may be NULL), sq[i] its squared norm (of the split values when norm_split != 0), Zh/Zl[i] (may be NULL) its bf16
 * hi/lo images with row stride kp.  The data-parallel step runs it for the NEXT batch while the gradient all-reduce is in
 * flight; the X-X tiles of the next Gram (sums only) then run behind the collective as well. */
int vgan_gather_rows_split(const float* data, int ldd, const int32_t* rows, const uint64_t* row_cursor,
                           int row_batches, int row_stride, int row_offset, const float* center, float* out,
                           int ldo, float* sq, int norm_split, uint16_t* Zh, uint16_t* Zl, int kp, int n, int d,
                           vgan_stream_t stream);
/* dlogits = softmax-Jacobian( [S < 1/d] * (gU + penalty_grad) ), the autograd of Generator.py:19-21.
 * colkey (may be NULL): packed column arg-max keys from vgan_colmax; row r of column j gets
 * -pen_weight/d added when it holds column j's maximum (topk(U,1,0), Mmd_loss_constrained.py:50). */
/* gU may be given as `nslabs` partial slabs `slab_stride` elements apart (split-K output of
 * vgan_mmd_backward); they are summed in ascending order inside the kernel. */
int vgan_mask_backward(const float* gU, int ldg, int nslabs, int64_t slab_stride, const float* S,
                       int lds, const uint64_t* colkey, float pen_weight, int row_offset,
                       float* dlogits, int ldo, int n, int d, vgan_stream_t stream);
/* colkey[j] = max over rows of pack(U[i,j], row_offset + i)  (value in the high 32 bits, ~row in
 * the low 32 bits; lowest row wins ties).  from_softmax != 0: the input is S and U is derived from
 * it; otherwise the input is U itself (must be > 0).  part: workspace [chunks*d] u64 with
 * chunks = vgan_colmax_chunks(n). */
int vgan_colmax_chunks(int n);
int vgan_colmax(const float* S, int lds, int from_softmax, int row_offset, uint64_t* part,
                uint64_t* colkey, int n, int d, vgan_stream_t stream);
/* first half of vgan_colmax only: per-chunk keys into part[chunks*d] (finished by vgan_mmd_finalize) */
int vgan_colmax_partial(const float* S, int lds, int from_softmax, int row_offset, uint64_t* part,
                        int n, int d, vgan_stream_t stream);
/* dense U from S (for callers that need the mask tensor itself) */
int vgan_mask_from_softmax(const float* S, int lds, float* U, int ldu, int n, int d, vgan_stream_t stream);
/* plain row softmax -> upper_softmax for a dense generator output (no projection) */
int vgan_upper_softmax_forward(const float* logits, int ldl, float* S, float* U, int n, int d,
                               vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * RBF + MMDLossConstrained  (src/models/Mmd_loss_constrained.py:16-26, 42-50)
 *
 * The 2n x 2n kernel matrix is never materialised.  The Gram tiles g = Z_I . Z_J^T run on the
 * fp32 MFMA; the epilogue forms L = |z_i|^2 + |z_j|^2 - 2g (clamped at 0), t = exp(-L/(4 bw)) and
 * the five-bandwidth sum K = t + t^2 + t^4 + t^8 + t^16, accumulates the block sums, and writes
 *     Wg[i - wrow0, j] = sgn(i,j) * (2/n^2) * dK/dL        (sgn = +1 same half, -1 across halves)
 * for the rows whose gradient is needed, so that  dZ_i = 2 (rowsum(Wg_i) z_i - (Wg . Z)_i).
 *
 * Work is described by a tile table (host-built by vgan_mmd_build_tiles, uploaded by the caller):
 * each entry is 8 int32 {r0, c0, rlim, clim, flags, 0,0,0}.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_TILE 64           /* Gram tile edge of the fp32 kernels; the split-bf16 Gram also has a 128 variant */
#define VGAN_TILE_INTS 8
#define VGAN_TF_SLOT_MASK 3    /* 0 = XX, 1 = XY, 2 = YY  block sum the tile contributes to */
#define VGAN_TF_TWICE 4        /* off-diagonal tile of a symmetric block: counted twice */
#define VGAN_TF_STORE 8        /* write Wg tile */
#define VGAN_TF_MIRROR 16      /* also write the transposed tile (symmetric block) */
#define VGAN_TF_NEG 32         /* sgn = -1 (rows and columns in different halves) */

/* grad_mode: 0 = no gradient (sums only), 1 = gradient for the Y rows only (Wg is [n, 2n],
 * wrow0 = n), 2 = gradient for all rows (Wg is [2n, 2n], wrow0 = 0).
 * Row-sharded data parallel: rank `rank` of `world` owns rows [rank*n/world, (rank+1)*n/world)
 * of each half; its table covers exactly the pairs (own row, any column), without symmetry.
 * tile: edge of the square tiles, 64 (every kernel) or 128 (vgan_mmd_gram_bf3 only), or 256 = tiles of 256 rows x 128 columns
 * (vgan_mmd_gram_bf3's loader-wave kernel; a symmetric block then keeps the two tiles of each 256 x 256 diagonal square whole and
 * mirrors / counts twice only the tiles outside it).
 * Row-sharded ranks (world > 1): (own Y rows) x (all columns) for the XY and YY blocks -- inside the rank's own diagonal YY block
 * the upper triangle with mirrored stores, when the block sits on the tile grid -- and, for the X-X block (sums only, no row
 * ownership), every world-th tile of the WHOLE block's upper triangle.
 * Returns the number of tiles (or -1 if cap is too small); out may be NULL to query the count. */
int vgan_mmd_build_tiles(int n, int grad_mode, int rank, int world, int tile, int32_t* out, int cap);
/* Re-applies the XCD-aware launch order (Morton curve, dealt to the 8 XCDs in contiguous chunks) to a table the caller
 * filtered or re-assembled on the host, e.g. the X-X tiles split off for the launch that overlaps the gradient all-reduce. */
int vgan_mmd_order_tiles(int32_t* tiles, int count, int tile);

/* partial[tiles*4] (float): per tile {sum K, sum L, 0, 0}.  calibrate != 0: only sum L is
 * produced (first-call bandwidth, Mmd_loss_constrained.py:16-20) and bw/Wg are not touched. */
int vgan_mmd_gram(const float* Z, int ldz, const float* sq, int n, int p, const float* bw,
                  const int32_t* tiles, int ntiles, int calibrate,
                  float* Wg, int ldw, int wrow0, float* partial, vgan_stream_t stream);
/* vgan_mmd_gram (calibrate = 0) for an RBF with other than the reference's defaults -- RBF(n_kernels, mul_factor),
 * Mmd_loss_constrained.py:7-13: K = sum_k exp(-L / (bw * multipliers[k])), one exp per kernel (the default
 * n_kernels = 5, mul_factor = 2 runs the one-exp squaring chain of vgan_mmd_gram).  multipliers is a HOST array of
 * n_kernels <= VGAN_RBF_MAX_KERNELS positive floats (mul_factor ** (k - n_kernels // 2)). */
#define VGAN_RBF_MAX_KERNELS 8
int vgan_mmd_gram_general(const float* Z, int ldz, const float* sq, int n, int p, const float* bw,
                          const int32_t* tiles, int ntiles, const float* multipliers, int n_kernels,
                          float* Wg, int ldw, int wrow0, float* partial, vgan_stream_t stream);
/* vgan_mmd_gram (calibrate = 0) and vgan_colmax_partial in ONE launch: the column arg-max cells run in surplus
 * workgroups behind the Gram tiles (they are independent of each other, and the Gram grid leaves CUs idle in its
 * tail).  Arguments as in the two separate calls; colpart has vgan_colmax_chunks(nrows)*d entries. */
int vgan_mmd_gram_colmax(const float* Z, int ldz, const float* sq, int n, int p, const float* bw,
                         const int32_t* tiles, int ntiles, float* Wg, int ldw, int wrow0, float* partial,
                         const float* S, int lds, int from_softmax, int row_offset, uint64_t* colpart,
                         int nrows, int d, vgan_stream_t stream);
/* stats[4] (double): {Sxx, Sxy, Syy, sumL} += reduction of partial[] by tile slot (deterministic).
 * zero_first != 0 clears stats before accumulating. */
int vgan_mmd_reduce(const float* partial, const int32_t* tiles, int ntiles, double* stats,
                    int zero_first, vgan_stream_t stream);
/* bw[0] = stats[3] / (N^2 - N), N = 2n   (Mmd_loss_constrained.py:18-19) */
int vgan_mmd_set_bandwidth(const double* stats, int n, float* bw, vgan_stream_t stream);
/* loss[0] = (Sxx - 2 Sxy + Syy)/n^2 + weight * mean_j(1 - colmax_j)   (Mmd_loss_constrained.py:47-50)
 * colkey may be NULL (weight term skipped).  loss_accum (may be NULL) += loss * accum_scale;
 * step_counter (may be NULL) += 1  (device-side step index for the Philox noise stream). */
int vgan_mmd_loss(const double* stats, const uint64_t* colkey, int n, int d, float weight,
                  float* loss, float* loss_accum, float accum_scale, uint64_t* step_counter,
                  vgan_stream_t stream);
/* Single-rank step tail in one launch = vgan_mmd_reduce (zero_first) + the second half of vgan_colmax
 * + vgan_mmd_loss: partial[] -> stats[4]; colpart[chunks*d] -> colkey[d] (colpart may be NULL: no
 * penalty term); loss / loss_accum / step_counter as in vgan_mmd_loss. */
int vgan_mmd_finalize(const float* partial, const int32_t* tiles, int ntiles, const uint64_t* colpart,
                      int chunks, uint64_t* colkey, int n, int d, float weight, double* stats,
                      float* loss, float* loss_accum, float accum_scale, uint64_t* step_counter,
                      vgan_stream_t stream);
/* The same step tail as a job that rides in a backward launch (vgan_mmd_backward / vgan_mmd_backward_bf3,
 * argument `finalize`, NULL = none): ONE extra workgroup of that launch does what vgan_mmd_finalize does, off
 * the critical path (its outputs -- colkey, the loss bookkeeping -- are first needed by the kernel AFTER the
 * backward product).  Field meaning as the arguments of vgan_mmd_finalize. */
typedef struct vgan_finalize_job {
    const float* partial;
    const int32_t* tiles;
    const uint64_t* colpart;
    uint64_t* colkey;
    double* stats;
    float* loss;
    float* loss_accum;
    uint64_t* step_counter;
    int32_t ntiles, chunks, n, d;
    float weight, accum_scale;
    /* mode 0: the whole tail.  Some X-X tiles of the Gram may be computed LATER in the step than the launch the tail rides in
     * (vgan_linear_backward_params_xx); the tail is then split: mode 1 = everything over the tiles [0, ntiles_main) (the Gram
     * launch's: all XY / YY tiles and any X-X tiles it had room for) -- column keys, block sums, the step counter; the loss so
     * far is parked in stats[3], the X-X sum so far in stats[0] -- and mode 2 = the X-X sums of the late tiles
     * [ntiles_main, ntiles), the loss and its accumulator (rides in vgan_gemm_grouped_ex, `fold`). */
    int32_t mode, ntiles_main;
} vgan_finalize_job;
/* dZ[i - wrow0, :] = 2 (rowsum(Wg_i) z_i - Wg_i . Z) for the nr rows starting at wrow0;
 * if mul != NULL the result is multiplied elementwise by mul[i - wrow0, :] (the `U * batch`
 * product rule: gU = dY * X).  Z is [ncols, p], Wg is [nr, ncols].
 * splits > 1: the contraction over the Z rows is cut into `splits` slices and slice s writes its
 * PARTIAL result to out + s*slab_stride (the result is linear in the slice sums); the consumer adds
 * the slabs (vgan_mask_backward does, or vgan_reduce_slabs).
 * mul_shift (may be NULL; needs mul): per-column constant added to mul, for callers whose Z (and with it the X rows
 * passed as `mul`) is stored centred: mul + mul_shift is then the batch itself.  Z may be centred freely: the
 * expression rowsum(Wg_i) z_i - Wg_i . Z = sum_j Wg_ij (z_i - z_j) is translation invariant. */
int vgan_mmd_backward(const float* Wg, int ldw, const float* Z, int ldz, int wrow0, int nr,
                      int ncols, int p, const float* mul, int ldmul, const float* mul_shift, float* out,
                      int ldo, int splits, int64_t slab_stride, const vgan_finalize_job* finalize,
                      vgan_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * Split-bf16 ("bf16x3") variants of the two dense contractions, for large problems (opt-in precision
 * mode): every operand z = hi + lo with hi = bf16(z), lo = bf16(z - hi), products hi.hi' + hi.lo' + lo.hi'
 * on the bf16 MFMA (16x the fp32 MFMA rate) with fp32 accumulation: ~3e-7 relative on a Gram entry at
 * K = 784.  The fused epilogues are those of the fp32 kernels.
 * ------------------------------------------------------------------------------------------- */
/* Z [rows, ldz] (first p columns) -> Zh, Zl [rows, kp] bf16 bit patterns (kp = p rounded up to 64, pad = 0)
 * and, unless NULL, the transposed images ZTh, ZTl [kp, kn] (kn = rows rounded up to 64, pad = 0). */
int vgan_mmd_bf3_prepare(const float* Z, int ldz, int rows, int p, uint16_t* Zh, uint16_t* Zl, int kp,
                         uint16_t* ZTh, uint16_t* ZTl, int kn, vgan_stream_t stream);
/* vgan_mmd_gram_colmax on the split operands; the gradient weights leave as a bf16 hi/lo pair Wh, Wl
 * [nr, ldw] (ldw >= 2n rounded up to 64 -- ldw % 8 == 0 and 16-byte aligned bases are checked: the epilogues store 16 bytes
 * at a time wherever the element offset allows; columns >= 2n must be pre-zeroed).  S may be NULL (no column job).
 * tile = the edge the table was built with: 64, 128 (512-thread workgroups, half the L2->LDS bytes per flop; pays when the
 * table still has >~ 128 tiles) or 256 (256 x 128 tiles, 768-thread workgroups of 8 consumer + 4 loader waves, three K stages
 * of 32 in LDS, v_mfma_f32_16x16x32_bf16: c4 / c5 sizes).
 * tail_ws (may be NULL; read only with tile = 256): device workspace of at least vgan_mmd_gram_bf3_tail_ws_bytes() bytes,
 * 16-byte aligned, whose last 4 096 bytes are ZERO before the first launch that uses it (the launches keep them zero) and
 * which no other launch uses concurrently.  With it, a table whose last round would leave at least half of the CUs idle (one
 * 768-thread workgroup holds a CU: ntiles mod CUs <= CUs / 2) has the tiles of that round computed by 2 or 4 workgroups
 * each, split over K; the partial products meet in the workspace and the last workgroup to arrive finishes the tile (sums in
 * part order: deterministic; nobody waits on anybody).  Results then differ from the unsplit launch by fp32 summation order
 * in those tiles only.
 * rs_part (may be NULL; tile = 256, n a multiple of 128, W stored): float [ceil(2n / 128), ldrs], ldrs >= rows of W.  Every
 * storing tile also leaves rs_part[c / 128][i - wrow0] = sum of the stored (hi + lo) weights of row i over the tile's columns
 * c .. c + 127 -- the row sums vgan_mmd_backward_bf3_rm needs, taken from the epilogue's registers.  Cells of slots no tile
 * covers are not written (zero them once). */
int64_t vgan_mmd_gram_bf3_tail_ws_bytes(void);
int vgan_mmd_gram_bf3(const uint16_t* Zh, const uint16_t* Zl, int kp, const float* sq, int n, const float* bw,
                      const int32_t* tiles, int ntiles, int tile, uint16_t* Wh, uint16_t* Wl, int ldw,
                      int wrow0, float* partial, const float* S, int lds, int from_softmax, int row_offset,
                      uint64_t* colpart, int nrows, int d, void* tail_ws, int64_t tail_ws_bytes,
                      float* rs_part, int ldrs, vgan_stream_t stream);
/* vgan_mmd_backward on the split operands: out = 2 (rowsum(W) z - W . Z) * mul with W = Wh + Wl [nr, kn]
 * and Z^T = ZTh + ZTl [kp, kn]; Z (fp32) is only read by the epilogue.  splits / slab_stride as in
 * vgan_mmd_backward (slabs of out, summed by the consumer in slab order); mul_shift as there.
 * tile: 0 = chosen by the library (256 x 128 loader-wave tiles once they fill the chip -- row-major B operand only --, else
 * 128-wide tiles once they fill it twice over, else 64), or 64 / 128 / 256 to force one. */
/* host-side query (no launch): the tile edge (64, 128 or 256) vgan_mmd_backward_bf3_rm uses for this shape and `tile` argument */
int vgan_mmd_backward_bf3_tile(int nr, int p, int splits, int tile);
int vgan_mmd_backward_bf3(const uint16_t* Wh, const uint16_t* Wl, int ldw, const uint16_t* ZTh,
                          const uint16_t* ZTl, int kn, int kp, const float* Z, int ldz, int wrow0, int nr,
                          int p, const float* mul, int ldmul, const float* mul_shift, float* out, int ldo,
                          int splits, int64_t slab_stride, int tile, const vgan_finalize_job* finalize,
                          vgan_stream_t stream);
/* The same backward product reading Z's ROW-MAJOR split images Zh, Zl [zrows, kp] -- the ones vgan_mmd_gram_bf3 reads -- so
 * that no transposed copy of Z has to be produced: the B fragments (8 consecutive contraction indices per lane) come out of a
 * row-major LDS image through ds_read_b64_tr_b16.  kn = the padded contraction length (columns of Wh / Wl, a multiple of 64,
 * >= zrows; columns >= zrows of W must be zero).  Everything else as vgan_mmd_backward_bf3.
 * rs_part (may be NULL): the per-slot row sums a tile-256 vgan_mmd_gram_bf3 launch left beside W (rs_part [ceil(kn / 128), ldrs],
 * ldrs >= nr).  The 256 x 128 kernel then folds them instead of having its loader waves sum the W rows from LDS (-5 % of the
 * launch at c5); ignored by the other tile sizes and when a K split is not a whole number of 128-column slots. */
int vgan_mmd_backward_bf3_rm(const uint16_t* Wh, const uint16_t* Wl, int ldw, int kn, const uint16_t* Zh,
                             const uint16_t* Zl, int kp, int zrows, const float* Z, int ldz, int wrow0, int nr,
                             int p, const float* mul, int ldmul, const float* mul_shift, float* out, int ldo,
                             int splits, int64_t slab_stride, int tile, const vgan_finalize_job* finalize,
                             const float* rs_part, int ldrs, vgan_stream_t stream);
/* vgan_mmd_backward_bf3_rm on 64-wide tiles with a few X-X tiles of the Gram (struct vgan_xx_job; identity row map) riding in
 * the launch as surplus workgroups: the backward launch of the training step fills 416 of the chip's 512 workgroup slots for
 * 25 us, so up to ~90 eight-microsecond tiles cost it nothing.  The tiles' partial sums are complete when the launch is;
 * a `finalize` job in the same launch must therefore not cover them (vgan_finalize_job.mode 1 / 2). */
int vgan_mmd_backward_bf3_rm_xx(const uint16_t* Wh, const uint16_t* Wl, int ldw, int kn, const uint16_t* Zh,
                                const uint16_t* Zl, int kp, int zrows, const float* Z, int ldz, int wrow0, int nr,
                                int p, const float* mul, int ldmul, const float* mul_shift, float* out, int ldo,
                                int splits, int64_t slab_stride, const vgan_finalize_job* finalize,
                                const struct vgan_xx_job* xx, vgan_stream_t stream);
/* The training step's form of that launch without an fp32 copy of Z: gU = 2 (rowsum(W) y - W . Z) * x for the nr batch rows,
 * where the epilogue forms its two operands itself instead of loading them from Z and `mul`:
 *     x = data[xrow[i], j],  c = center[j],  u = S[i, j] < 1/p ? S[i, j] : 1,
 *     y = fma(u, x, -c)  (the Y row vgan_mask_project_forward_bf3 writes),  multiplier = fl(fl(x - c) + c)  (mul + mul_shift).
 * Bit for bit the result of vgan_mmd_backward_bf3_rm_xx called with the Z that vgan_mask_project_forward_bf3 wrote from the same
 * data rows, S and centre, mul = its X half and mul_shift = center -- so the mask / projection launch need not write Z at all
 * (vgan_mask_project_forward_bf3_ex, write_z = 0: 6.4 of its 22.8 MB per step at n = 1024, d = 784).  64-wide tiles;
 * xrow: int32 [nr] as that launch leaves it; S: [nr, lds] with p columns; xx and finalize may be NULL. */
typedef struct vgan_bwd_rebuild {
    const float* data;   /* the data set [rows, ldd] */
    const int32_t* xrow; /* [nr] data-set row of each batch row */
    const float* S;      /* [nr, lds] softmax rows */
    const float* center; /* [p] */
    int32_t ldd, lds;
} vgan_bwd_rebuild;
int vgan_mmd_backward_bf3_rm_rebuild(const uint16_t* Wh, const uint16_t* Wl, int ldw, int kn, const uint16_t* Zh,
                                     const uint16_t* Zl, int kp, int zrows, int nr, int p,
                                     const vgan_bwd_rebuild* rebuild, float* out, int ldo, int splits,
                                     int64_t slab_stride, const vgan_finalize_job* finalize,
                                     const struct vgan_xx_job* xx, vgan_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * Grouped small products: up to VGAN_GEMM_MAX_GROUP independent row-major GEMMs in one launch.
 * Generator_big (src/models/Generator.py:61-66) has no activation between its Linear layers, so its
 * forward/backward is a chain of small matrix products (see vgan_homogeneous_pack); products of one
 * dependency level share a launch.  kind: NN C[m,n] = A[m,k] . B[k,n];  NT C = A[m,k] . B[n,k]^T;
 * TN C = A[k,m]^T . B[k,n].  All operands row-major with leading dimensions lda / ldb / ldc.
 * splitk > 1: the contraction is cut into splitk slices run by different workgroups (for a long contraction over few
 * output tiles); slice s writes its PARTIAL product to slab s of C, slabs m * ldc floats apart, and the caller sums the
 * slabs in fixed order (vgan_reduce_slabs) -- deterministic, so data-parallel replicas stay bit-identical.  0 / 1: no split.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_GEMM_MAX_GROUP 4
#define VGAN_GEMM_NN 0
#define VGAN_GEMM_NT 1
#define VGAN_GEMM_TN 2
#define VGAN_GEMM_NT_NT 3 /* two products in one tile: C[m,n] = (A[m,k] . B[k2,k]^T) . D[n,k2]^T -- a 64 x 64 tile of C first forms its 64
                           * rows of H = A . B^T ([64, k2], into `scratch`: ceil(m/64) * ceil(n/64) regions of 64 * round4(k2)
                           * floats, one per tile) and then multiplies them with D.  For a dependent pair of small products whose
                           * second would otherwise cost a launch of its own (the logits of the collapsed generator: T = ([z|1] .
                           * Wt_1^T) . Wt_2^T rides with the first level of chain products, src/models/Generator.py:61-66). */
typedef struct vgan_gemm_problem {
    const float* a;
    const float* b;
    float* c;
    int32_t kind, m, n, k, lda, ldb, ldc, splitk;
    const float* d;   /* VGAN_GEMM_NT_NT only */
    float* scratch;   /* VGAN_GEMM_NT_NT only */
    int32_t ldd, k2;  /* VGAN_GEMM_NT_NT only: D [n, k2] row-major */
} vgan_gemm_problem;
int vgan_gemm_grouped(const vgan_gemm_problem* problems, int count, vgan_stream_t stream);
/* The same launch with work riding in it (each part optional; a dependent launch costs ~5 us whatever its size, so the
 * tail of the step shares launches):
 *   copy      dst[i] = src[i], i < copy_count (a snapshot a later launch of the step reads while its source is updated);
 *   adadelta  != 0: problem i's output C_i is the packed gradient [dW | db] of layer[i] (rows < out, columns <= in, column
 *             `in` = bias) and the torch.optim.Adadelta update (src/vgan.py:567-568, :619; rule of vgan_adadelta_step) runs in
 *             the product's epilogue: the flat parameter p[off_w + row*in + col] / p[off_b + row], its state, and the packed
 *             weight w_packed[row*ldp + col] are updated in place (C_i is still written).  None of the launch's operands
 *             may alias an updated w_packed.  g_extra != NULL: one more layer, layer[count], whose packed gradient already
 *             sits in memory (row stride ld_extra) is updated element-wise by surplus workgroups;
 *   noise     next_noise != NULL: the next step's noise draw, as in vgan_adadelta_step_packed;
 *   fold      a vgan_finalize_job run by one surplus workgroup (the late half of a split step tail). */
typedef struct vgan_adadelta_layer {
    float* w_packed;
    int64_t off_w, off_b;
    int32_t ldp, out, in, pad;
} vgan_adadelta_layer;
typedef struct vgan_grouped_extras {
    const float* copy_src;
    float* copy_dst;
    int64_t copy_count;
    int32_t adadelta, pad;
    float* p;
    float* sq_avg;
    float* acc_delta;
    float lr, rho, eps, weight_decay, grad_scale;
    int32_t ld_extra;
    vgan_adadelta_layer layer[VGAN_GEMM_MAX_GROUP + 1];
    const float* g_extra;
    float* next_noise;
    int32_t noise_rows, noise_cols, noise_ld, noise_ones_col;
    uint64_t seed;
    const uint64_t* step_counter;
    const vgan_finalize_job* fold; /* NULL, or a step-tail job (normally mode 2) run by one surplus workgroup */
} vgan_grouped_extras;
int vgan_gemm_grouped_ex(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras,
                         vgan_stream_t stream);
/* vgan_gemm_grouped_ex with an in-launch K split per problem: kparts[i] (1..8) workgroups share each 32 x 32 tile of problem
 * i and combine inside the launch as in vgan_linear_backward_params_ksplit (same workspace rules; the tickets, one int32 per tile
 * of the split problems in problem order, lead the workspace).  kparts == NULL or all 1: exactly vgan_gemm_grouped_ex.  Otherwise
 * the launch must be one the library runs on its 16-wave 32 x 32 tiles (every k >= 96, at most 256 tiles in all, the vector
 * contract, no optimiser epilogue, no noise job; copy and fold jobs may ride) -- anything else is VGAN_ERR_ARG, as is kparts[i] > 1
 * together with splitk > 1 (that form writes slabs of C for vgan_reduce_slabs).  extras may be NULL. */
/* Host-side path query of the grouped launches (see vgan_linear_forward_path): the launch vgan_gemm_grouped (extras and kparts
 * NULL), vgan_gemm_grouped_ex (kparts NULL) or vgan_gemm_grouped_ksplit makes for these arguments, or a negative value where
 * they return VGAN_ERR_ARG (the K split's workspace, which the query is not given, aside).  The code names the launch, its vector
 * width and whether the optimiser epilogue is instantiated; engine (may be NULL) receives the tile engine of each problem.
 * The operand pointers inside `problems` are only tested for nullness and alignment. */
enum vgan_gemm_grouped_path_code {
    VGAN_GEMM_GROUPED_T256_V4 = 0,     /* gemm_grouped_kernel<4, false>: 256 threads, per problem 64 x 64 or 4-wave 32 x 32 tiles */
    VGAN_GEMM_GROUPED_T256_V4_EPI = 1, /* gemm_grouped_kernel<4, true>: with the optimiser epilogue */
    VGAN_GEMM_GROUPED_T256_V1 = 2,     /* gemm_grouped_kernel<1, false> */
    VGAN_GEMM_GROUPED_T256_V1_EPI = 3, /* gemm_grouped_kernel<1, true> */
    VGAN_GEMM_GROUPED_KS16 = 4,        /* gemm_grouped_ks16_kernel: every problem on 16-wave 32 x 32 tiles (vector width 4) */
    VGAN_GEMM_GROUPED_KS16_SPLIT = 5,  /* gemm_grouped_ks16_split_kernel: the same with the in-launch K split */
    VGAN_GEMM_GROUPED_PATHS = 6
};
enum vgan_gemm_engine {
    VGAN_GEMM_ENGINE_T64 = 0, /* 64 x 64 x 32 tiles (also VGAN_GEMM_NT_NT and every problem with splitk > 1) */
    VGAN_GEMM_ENGINE_KS4 = 1, /* 32 x 32 tiles, 4 waves: k >= 128 and at most 512 such tiles */
    VGAN_GEMM_ENGINE_KS16 = 2 /* 32 x 32 tiles, 16 waves: every problem of a KS16 launch */
};
int vgan_gemm_grouped_path(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras, const int32_t* kparts,
                           int32_t* engine /* [count] */);
int64_t vgan_gemm_grouped_ksplit_ws_bytes(const vgan_gemm_problem* problems, int count, const int32_t* kparts);
int vgan_gemm_grouped_ksplit(const vgan_gemm_problem* problems, int count, const vgan_grouped_extras* extras,
                             const int32_t* kparts, void* ws, int64_t ws_bytes, vgan_stream_t stream);

/* vgan_mask_project_forward fused with vgan_mmd_bf3_prepare for the training step: from logits [n, d] and the
 * batch rows it writes S [n, d], Z = [X ; U*X] ([2n, ldz] fp32), sq [2n] and the split images Zh, Zl [2n, kp],
 * ZTh, ZTl [kp, kn] of Z (pad regions are not touched: pre-zeroed by the caller).  Shape contract: d % 4 == 0,
 * d <= 1024, n % 8 == 0, leading dimensions % 4 == 0, 16-byte aligned bases; otherwise use the two calls
 * (with norm_split = 1).  center as in vgan_mask_project_forward; sq holds the norms of the split values.
 * ZTh / ZTl may both be NULL (callers of vgan_mmd_backward_bf3_rm need no transposed images).
 * write_x == 0 (needs ZTh == NULL): the X half of Z, sq, Zh, Zl is left alone -- vgan_gather_rows_split has already produced
 * it for this batch.
 * xx (may be NULL; needs ZTh == NULL): the X-X tiles of the Gram ride in this launch as surplus workgroups.  They only
 * feed the block sum of the reported loss and depend on nothing the step computes: their operand is this batch's rows of
 * the data set, gathered by the same index table from split images prepared once per fit -- Dh, Dl [data rows, ldd] and dsq
 * (vgan_gather_rows_split over the whole data set with norm_split = 1).  tiles / ntiles: the X-X part of the tile table
 * (vgan_mmd_build_tiles, flags slot 0); partial: where their sums go (4 floats per tile, the layout vgan_mmd_finalize folds);
 * bw: the frozen bandwidth.  The Gram launch then covers the XY and YY tiles only.
 * chain (may be NULL; needs ZTh == NULL): as in vgan_mask_project_forward.
 * vgan_mask_project_forward_bf3_ex: the same launch with two more arguments.  write_z == 0: the fp32 operand Z is not written
 * (Z may be NULL; S, sq and the split images are written as always) -- for steps whose backward is
 * vgan_mmd_backward_bf3_rm_rebuild.  xrow (may be NULL): int32 [n], receives the data-set row of every batch row.
 * Without ZTh, xx and chain and with 256 < d <= 1024 the launch runs one batch row per workgroup (d / 256 rounded up waves)
 * instead of one per wave; every output is bit for bit the same. */
typedef struct vgan_xx_job {
    const uint16_t* Dh;
    const uint16_t* Dl;
    const float* dsq;
    const int32_t* tiles;
    const float* bw;
    float* partial;
    int32_t ldd, ntiles;
} vgan_xx_job;
int vgan_mask_project_forward_bf3(const float* logits, int ldl, const float* data, int ldd, const int32_t* rows,
                                  const uint64_t* row_cursor, int row_batches, int row_stride, float* S, float* Z,
                                  int ldz, float* sq, uint16_t* Zh, uint16_t* Zl, int kp, uint16_t* ZTh,
                                  uint16_t* ZTl, int kn, int n, int d, const float* center, int write_x,
                                  const vgan_xx_job* xx, const vgan_logits_chain* chain, vgan_stream_t stream);
int vgan_mask_project_forward_bf3_ex(const float* logits, int ldl, const float* data, int ldd, const int32_t* rows,
                                     const uint64_t* row_cursor, int row_batches, int row_stride, float* S, float* Z,
                                     int ldz, float* sq, uint16_t* Zh, uint16_t* Zl, int kp, uint16_t* ZTh,
                                     uint16_t* ZTl, int kn, int n, int d, const float* center, int write_x,
                                     const vgan_xx_job* xx, const vgan_logits_chain* chain, int write_z, int32_t* xrow,
                                     vgan_stream_t stream);
/* squared row norms sq[r] = |Z_r|^2 (for callers that assemble Z themselves) */
int vgan_row_sqnorm(const float* Z, int ldz, float* sq, int rows, int p, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch.optim.Adadelta over one flat parameter buffer  (src/vgan.py:567-568, :619)
 *   g += wd*p; v = rho v + (1-rho) g^2; delta = sqrt(a+eps)/sqrt(v+eps) g; a = rho a + (1-rho) delta^2;
 *   p -= lr*delta.   grad_scale multiplies g first (1 for plain training).  g may be `nslabs` split-K
 *   slabs `slab_stride` elements apart (see vgan_linear_backward_params): summed in ascending order.
 * ------------------------------------------------------------------------------------------- */
int vgan_adadelta_step(float* p, const float* g, int nslabs, int64_t slab_stride, float* sq_avg,
                       float* acc_delta, int64_t count, float lr, float rho, float eps,
                       float weight_decay, float grad_scale, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Noise feed  (src/vgan.py:610 `noise_tensor.normal_()`): standard normals from a counter-based
 * Philox4x32-10 stream + Box-Muller, keyed by (seed, *step_counter); replay-safe under HIP graphs.
 * ------------------------------------------------------------------------------------------- */
/* z is [rows, cols] with row stride ld; element (r,c) is draw number r*cols + c of the stream, so the
 * values do not depend on ld.  ones_col >= cols (or -1): column that is set to 1.0 in every row (the
 * homogeneous coordinate of the collapsed generator chain). */
int vgan_noise_normal(float* z, int rows, int cols, int ld, int ones_col, uint64_t seed,
                      const uint64_t* step_counter, uint64_t stream_id, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Generator_big has NO activation between its four Linear layers (src/models/Generator.py:61-66),
 * so in homogeneous coordinates the chain is a product of matrices Wt_k = [[W_k, b_k],[0, 1]]:
 *   logits = [z|1] . (Wt_4 Wt_3 Wt_2 Wt_1)^T   and   dWt_k = (Wt_{k+1..4}^T dlogits^T [z|1]) . (Wt_{k-1..1})^T,
 * i.e. every product has an inner or outer dimension of L+1 instead of the batch: ~0.2 GFLOP instead
 * of 2.5 GFLOP per step at d=784.  The products run on vgan_linear_*; this entry point moves the
 * parameters/gradients between the PyTorch layout and the packed one in a single launch.
 * desc: device table, 8 int64 per layer {W ptr, b ptr, packed ptr, out, in, ldw, ldp, 0};
 * packed is [out+1, in+1] with row stride ldp.  unpack != 0: packed -> (W, b) (rows < out only).
 * max_elems: the largest (out+1)*(in+1) in the table (sizes the grid). */
int vgan_homogeneous_pack(const int64_t* desc, int count, int max_elems, int unpack, vgan_stream_t stream);
/* Adadelta for that chain without pack/unpack launches: the gradient of flat element i is
 * g_packed[pmap[i]] and the updated parameter is also stored to w_packed[pmap[i]] (pmap[i] < 0: layout
 * padding, skipped).  Same update rule as vgan_adadelta_step.
 * next_noise != NULL: the kernel also draws the noise of the NEXT step (vgan_noise_normal with
 * stream_id 0 and the current value of *step_counter, which the loss kernel has already advanced),
 * saving the separate noise launch at the head of every step. */
int vgan_adadelta_step_packed(float* p, const int32_t* pmap, const float* g_packed, float* w_packed,
                              float* sq_avg, float* acc_delta, int64_t count, float lr, float rho,
                              float eps, float weight_decay, float grad_scale, float* next_noise,
                              int noise_rows, int noise_cols, int noise_ld, int noise_ones_col,
                              uint64_t seed, const uint64_t* step_counter, vgan_stream_t stream);

/* sum of squared differences: out[0] (+)= scale * sum((a-b)^2)  -- `__distance(x,y,'L2')`,
 * src/vgan.py:58-59 (one workgroup; for reporting-sized inputs). */
int vgan_mse(const float* a, int lda, const float* b, int ldb, int n, int d, float scale,
             float* out, int accumulate, vgan_stream_t stream);

/* The same term with its gradient, for VGAN.fit's detector loss (src/vgan.py:276-277): one pass over [n, d],
 * part[b] (b < ceil(n/4)) = float64 partial sums of (pred - target)^2, g = gscale * (pred - target).
 * vgan_sum_f64 folds such partials: out[0] (+)= scale * sum(in[0..count)), fixed order. */
int vgan_mse_grad(const float* target, int ldt, const float* pred, int ldp, int n, int d, float gscale,
                  double* part, float* g, int ldg, vgan_stream_t stream);
int vgan_sum_f64(const double* in, int count, double scale, float* out, int accumulate, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Data-parallel exchange  (the reference has no collective): thin wrappers over RCCL for callers that do not
 * use torch.distributed.  One process per GPU.  Rank 0 calls vgan_dp_unique_id and hands the 128 bytes to every rank by
 * its own means; each rank then creates its communicator and, once per step, all-reduces (SUM, in place, float32) the
 * generator gradient on the stream the step's kernels run on -- after vgan_linear_backward_params has produced M_4 (or the
 * flat gradient), before the products that consume it.  To overlap it, issue it on a second stream and run
 * vgan_gather_rows_split + the X-X tiles of the next batch meanwhile (what v-gan_amd/trainer.py does).
 * RCCL is dlopen'ed at first use: without librccl.so these calls return VGAN_ERR_HIP and everything else still works.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_DP_ID_BYTES 128
typedef struct vgan_dp_comm vgan_dp_comm;
int vgan_dp_unique_id(uint8_t* id /* [VGAN_DP_ID_BYTES] */);
int vgan_dp_comm_create(vgan_dp_comm** comm, int nranks, const uint8_t* id, int rank);
int vgan_dp_allreduce_sum(vgan_dp_comm* comm, float* buf, int64_t count, vgan_stream_t stream);
/* In-place all-gather of raw bytes: rank r's bytes_per_rank bytes already sit at buf + r * bytes_per_rank; afterwards every rank
 * holds all nranks pieces.  The exchange of the SHARDED front of a data-parallel step (chosen for large
 * batches, v-gan_amd/trainer.py): each rank runs vgan_linear_forward, vgan_mask_project_forward(row_offset = its first row),
 * vgan_mmd_bf3_prepare and vgan_colmax_partial for ITS rows only, then the ranks gather the Y rows of the split images (or of
 * Z in fp32 mode), their norms and the column-key chunks -- three or four calls, or one over a packed record -- while the
 * Gram tiles that need no other rank's rows (XY, X-X) run on another stream.
 * STATUS of the four vgan_dp_* calls: exercised on MI355X with nranks = 1 only (a one-GPU box cannot form a larger
 * communicator); the Python engine carries the same exchanges through torch.distributed (backend "nccl" = RCCL). */
int vgan_dp_allgather(vgan_dp_comm* comm, void* buf, int64_t bytes_per_rank, vgan_stream_t stream);
int vgan_dp_comm_destroy(vgan_dp_comm* comm);

/* ---------------------------------------------------------------------------------------------
 * Input pipeline / sampling post-processing on the device  
 * vgan_shuffle_epoch: perm[i] = pi_{seed,epoch}(i) for i < count, pi a pseudo-random permutation of [0, train_size)
 * evaluated per element (balanced Feistel network + cycle walking): the shuffled drop_last batches of one epoch
 * (DataLoader(shuffle=True, drop_last=True), src/vgan.py:578-584) without a host draw, a sort or a copy.  It is NOT torch's
 * randperm stream: parity runs keep the host draw.  vgan_shuffle_index evaluates the same permutation on the host.
 * vgan_mask_unique: np.unique(masks, axis=0, return_counts=True) of approx_subspace_dist (src/vgan.py:372-382) for a
 * boolean (uint8) mask matrix [n, d]: out_row[r] = index of the first sampled row holding the r-th distinct mask in
 * numpy's lexicographic order, out_count[r] = its multiplicity; entries r >= #distinct are left untouched (pre-zero
 * out_count).  keys: workspace [n * ceil(d/64)] u64, work: [2n] i32.
 * ------------------------------------------------------------------------------------------- */
int vgan_shuffle_epoch(int32_t* perm, int64_t count, int64_t train_size, uint64_t seed, uint64_t epoch,
                       vgan_stream_t stream);
int64_t vgan_shuffle_index(int64_t i, int64_t train_size, uint64_t seed, uint64_t epoch);
int vgan_mask_unique(const uint8_t* masks, int ldm, int n, int d, uint64_t* keys, int32_t* work,
                     int32_t* out_row, int32_t* out_count, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Myopicity two-sample test  (check_if_myopic, src/vgan.py:384-431 -> torch-two-sample's MMDStatistic
 * with ret_matrix=True and its permutation p-value; that dependency is absent and unpinned, the algorithm
 * is restated in oracle/vgan_oracle.py: PARITY UNPINNED against the dependency).
 * vgan_rbf_kernel_matrix: K[i,j] = exp(-alpha |z_i - z_j|^2) for the m rows of Z ([m, p], sq = squared row
 * norms), K[i,i] = 1.   vgan_rows_dot: out[r] = sum_c A[r,c] * B[r*ldb + c] in float64 (ldb = 0 broadcasts
 * one row of B) -- with T = Ut . K (vgan_gemm_grouped) this gives u^T K u and u^T K 1 for every 0/1
 * assignment row u of Ut, from which the host forms the permutation statistics.
 * ------------------------------------------------------------------------------------------- */
int vgan_rbf_kernel_matrix(const float* Z, int ldz, int m, int p, const float* sq, float alpha, float* K, int ldk,
                           vgan_stream_t stream);
/* RBF.forward(Z) -> K [m, m]  (src/models/Mmd_loss_constrained.py:24-26) for callers of the stand-alone module:
 * K[i,j] = sum_k exp(-|z_i - z_j|^2 / (bw[0] * multipliers[k])); bw is a DEVICE scalar (the frozen bandwidth),
 * multipliers a HOST array.  dK (may be NULL) receives dK/dL = -sum_k exp(..)/(bw multipliers[k]), what the module's
 * autograd multiplies the upstream gradient with before vgan_mmd_backward. */
int vgan_rbf_multi_kernel_matrix(const float* Z, int ldz, int m, int p, const float* sq, const float* bw,
                                 const float* multipliers, int n_kernels, float* K, int ldk, float* dK, int lddk,
                                 vgan_stream_t stream);
int vgan_rows_dot(const float* A, int lda, const float* B, int ldb, double* out, int rows, int cols,
                  vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Outlier scoring over generated subspaces  (v-gan_amd/outlier.py: SubspaceEnsemble; the use the reference
 * README gives the learnt subspaces, "ensembling in the Outlier Detection problem", with pyod's KNN / LOF /
 * KDE as the base detectors).  A SUBSPACE TABLE is three device arrays over S subspaces:
 *   feat      int32, the feature indices of every subspace, concatenated;
 *   feat_off  int32 [S+1], subspace s holds feat[feat_off[s] .. feat_off[s+1]), d_s of them (d_s >= 1);
 *   col_off   int64 [S+1], col_off[s] = sum_{t<s} w_t with w_t = round4(d_t): the packed column offsets.
 * A call covers the subspaces [first, first + count) of the table (a chunk).  The PACKED block of a row set of
 * n rows holds, for chunk subspace s, the rows [n, w_s] row-major at element n * (col_off[s] - col_off[first]).
 * Neighbour order everywhere is the strict total order (distance, reference index).
 * vgan_outlier_pack: the packed block of X [n, d] (ldx): X[i, feat] - center[feat] (center may be NULL: not centred), zero
 *   padded to w_s; sq (may be NULL) [count, n] receives the squared row norms of the packed values.
 * vgan_outlier_knn: for every chunk subspace and query row q < nq, the k reference rows nearest in the packed blocks Pq / Pr,
 *   nbr [count, nq, k] int32 in (engine distance, index) order.  engine VGAN_OUTLIER_ENGINE_EXACT sums (q_f - r_f)^2 on the
 *   vector ALU (sq_q / sq_r unused); VGAN_OUTLIER_ENGINE_GRAM forms |q|^2 + |r|^2 - 2 q.r with the fp32 MFMA (needs sq_q /
 *   sq_r; give it centred blocks).  exclude_self != 0: the query set IS the reference set (nq == nr) and row q never lists
 *   itself (exact duplicates of it stay).  splits J > 1 cuts the reference rows into J slices; slice lists go to the
 *   workspaces part_d / part_i [count, J, nq, k] and a second launch merges them.  The result is the same for every J.
 *   1 <= k <= VGAN_OUTLIER_MAX_K, nr >= k (+1 when self is excluded).
 * vgan_outlier_refine: the k neighbours of nbr re-measured in float64 from the raw rows Xq [nq, d] / Xr [nr, d] over each
 *   subspace's features, re-sorted by (float32 distance, index): out_idx / out_dist [count, nq, k]; kdist (may be NULL)
 *   [count, nq] receives the k-th distance.
 * vgan_outlier_score: from sorted lists (idx, dist) [count, nq, k]:
 *   VGAN_OUTLIER_KNN_LARGEST / _MEAN / _MEDIAN  score[row, q] = k-th / mean / median distance;
 *   VGAN_OUTLIER_LRD   lrd_out [count, nq] (float64) = 1 / (mean_o max(kdist_ref[o], dist(q, o)) + 1e-10);
 *   VGAN_OUTLIER_LOF   score[row, q] = mean_o lrd_ref[o] / lrd(q)  (sklearn's LocalOutlierFactor, positive: larger is
 *                      more outlying; kdist_ref [count, nr] float32, lrd_ref [count, nr] float64 of the reference rows).
 *   row = score_row[z] for chunk subspace z (score_row: device int32 [count], may be NULL: row = z); ld_score >= nq.
 * vgan_outlier_kde: Gaussian kernel density of every query row q < nq among the reference rows in each chunk subspace,
 *   score[row, q] = -log p_s(q) (float32; row and ld_score as for vgan_outlier_score), with p_s from the packed blocks
 *   Pq / Pr and the engines of vgan_outlier_knn (same sq_q / sq_r rules):
 *     log p_s(q) = logsumexp_r(-d2(q, r) / (2 h_s^2)) - log N - d_s log h_s - d_s / 2 log(2 pi).
 *   bandwidth: device float64 [S], h_s by table position (processing order), finite and > 0.  exclude_self != 0: the
 *   query set IS the reference set (nq == nr >= 2), row q's own index is left out and N = nr - 1 (exact duplicates of it
 *   stay); otherwise N = nr.  Workspaces pivot uint32 [count, nq] and acc uint64 [count, nq] are initialised by the call.
 *   Three sweeps: the per-row minimum d2 (pivot), sum_r exp2(c_s (pivot - d2)) in uint64 fixed point at 2^-40 (every term
 *   <= 1, so nothing underflows to -inf; integer atomics, so the result is the same for every J), the float64 score.
 *   nr <= VGAN_OUTLIER_KDE_MAX_ROWS keeps the fixed-point sum below 2^63.
 * vgan_outlier_combine: out[i] = sum_s weights[s] * score[s, i] for s = 0 .. S-1 in that order, float64.
 * vgan_outlier_score_stats: a centre and a scale (float64 [S]) per row of the finished score matrix [S, ld] (n scores a
 *   row, float32, taken as float64).  Row s is whatever the caller stored there: the call knows no subspace table, and
 *   center[s] / scale[s] belong to row s (SubspaceEnsemble keeps the matrix in the given subspace order).
 *     VGAN_OUTLIER_NORM_ZSCORE  mean; population standard deviation sqrt(mean((x - center)^2)), two passes
 *     VGAN_OUTLIER_NORM_ROBUST  median (even n: half the sum of the two middle order statistics);
 *                               median(fabs(x - center)) / 0.6744897501960817, fabs(x - center) formed in float64
 *     VGAN_OUTLIER_NORM_MINMAX  minimum; maximum - minimum
 *   A scale that would be 0 is 1.  The order statistics are exact (a segmented radix select on integer counts), the
 *   moments fixed-shape float64 reductions without float atomics: every output is bit-identical from run to run.
 *   Non-finite scores leave the statistics unspecified (no fault).  workspace: device memory, 16-byte aligned, of at
 *   least vgan_outlier_score_stats_ws_bytes(S, n, mode) bytes (-1 for bad arguments), initialised by the call.
 *   1 <= S <= 65535, 1 <= n <= ld.
 * vgan_outlier_combine_normalized: with t_s(x) = (double(x) - center[s]) / scale[s] (center and scale both NULL: t_s(x) =
 *   double(x)), out[i] = sum_s weights[s] * t_s(score[s, i]) (VGAN_OUTLIER_COMBINE_SUM, s = 0 .. S-1 in that order) or
 *   max_s t_s(score[s, i]) (VGAN_OUTLIER_COMBINE_MAX; weights unused, may be NULL), float64.
 * vgan_outlier_abod: angle-based outlier scores (FastABOD: Kriegel, Schubert, Zimek 2008; pyod's ABOD, method="fast") from
 *   the refined lists idx [count, nq, k] of vgan_outlier_refine and the raw rows Xq [nq, d] (ldq) / Xr [nr, d] (ldr).  For
 *   chunk subspace s, query row q and each listed reference row a: v_a = Xr[a, F_s] - Xq[q, F_s] in float64 (exact), n_a =
 *   |v_a|^2; a is usable if n_a > 0 (an entry outside [0, nr) is not).  Over the unordered pairs of usable neighbours,
 *   w_ab = <v_a, v_b> / (n_a n_b), and score[row, q] = -var(w): the population variance, two passes (mean, then mean
 *   squared deviation) in float64 in a fixed order, stored as float32 (row and ld_score as for vgan_outlier_score); a
 *   result below the float32 range is stored as -FLT_MAX.  One pair gives 0.  A row with fewer than two usable
 *   neighbours is DEGENERATE and its score is stored as NaN, for vgan_outlier_abod_floor.  The lists decide the bits:
 *   the same lists give the same scores in every run and for every chunking.  2 <= k <= VGAN_OUTLIER_MAX_K, nr >= k.
 * vgan_outlier_abod_floor: on the finished score matrix [S, ld] (n scores a row), row by row.  fit != 0: score_floor[s]
 *   (float64 [S]) = the smallest score of row s that is not NaN, 0 if every score is NaN; n_degenerate[s] (int32 [S]) =
 *   the number of NaN scores.  fit == 0: score_floor is read, n_degenerate is not touched (may be NULL).  Then every NaN
 *   of row s becomes (float)score_floor[s].  The call knows no subspace table: row s is whatever the caller stored there.
 * vgan_outlier_cof_chain: the average chaining distance of the connectivity-based outlier factor (COF: Tang, Chen, Fu, Cheung
 *   2002; pyod's COF) from the refined lists idx [count, nq, k] of vgan_outlier_refine and the raw rows Xq / Xr.  For chunk
 *   subspace s and query row q let o_0 = q and o_1 .. o_k the listed reference rows in list order.  d2(a, b) = sum_{f in F_s}
 *   (x_a[f] - x_b[f])^2 in float64 from the raw float32 values, features ascending, differences per feature (never
 *   n_a + n_b - 2 G_ab).  chain VGAN_OUTLIER_COF_CHAIN_SBN (the paper's set-based nearest path): the set starts as {o_0};
 *   step i = 1 .. k adds the remaining point with the smallest (d2 to the set, list position), where the d2 of a point to
 *   the set is its minimum d2 over the set's members, and e_i = sqrt of that d2; the comparisons are made on d2 and a tie
 *   goes to the lower list position.  VGAN_OUTLIER_COF_CHAIN_RANK: e_i = sqrt(min_{j < i} d2(o_i, o_j)), the points in list
 *   order.  ac_out[z, q] (float64 [count, nq]) = sum_{i = 1 .. k} w_i e_i with w_i = 2 (k + 1 - i) / (k (k + 1)), float64,
 *   i ascending, no atomics: the lists decide the bits.  An entry outside [0, nr) counts as a point at the origin (the
 *   lists of vgan_outlier_refine hold none).  1 <= k <= VGAN_OUTLIER_MAX_K, nr >= k.
 * vgan_outlier_cof_score: score[row, q] = ac_q[z, q] k / sum_{i = 1 .. k} ac_ref[z, idx[z, q, i]] (ac_q float64 [count, nq],
 *   ac_ref float64 [count, nr]: the chaining distances of the reference rows at fit, self excluded), float64, i
 *   ascending, stored as float32 (row and ld_score as for vgan_outlier_score); a value beyond the float32 range is stored
 *   as FLT_MAX.  A zero denominator: the score is exactly 1 where ac_q is 0 too (a point mass among point masses: not
 *   degenerate); where ac_q > 0 the row is DEGENERATE and its score is stored as NaN, for vgan_outlier_cof_ceiling.
 * vgan_outlier_cof_ceiling: vgan_outlier_abod_floor with a maximum.  fit != 0: score_ceiling[s] (float64 [S]) = the largest
 *   score of row s that is not NaN, 1 if every score is NaN; n_degenerate[s] (int32 [S]) = the number of NaN scores.
 *   fit == 0: score_ceiling is read, n_degenerate is not touched (may be NULL).  Then every NaN of row s becomes
 *   (float)score_ceiling[s].
 * Other metrics of the neighbour search (kNN, LOF, kneighbors).  Over F_s, on the raw float32 features taken as float64:
 *     VGAN_OUTLIER_METRIC_EUCLIDEAN  sqrt(sum_f (x_f - y_f)^2): the entries above
 *     VGAN_OUTLIER_METRIC_MANHATTAN  sum_f |x_f - y_f|
 *     VGAN_OUTLIER_METRIC_CHEBYSHEV  max_f |x_f - y_f|
 *     VGAN_OUTLIER_METRIC_MINKOWSKI  (sum_f |x_f - y_f|^p)^(1/p), p finite in (0, VGAN_OUTLIER_MAX_P]; p < 1 is allowed
 *                                    and is not a metric (no triangle inequality)
 *     VGAN_OUTLIER_METRIC_COSINE     1 - <x, y> / (|x| |y|), not centred; exactly 1 when |x| or |y| is 0 (scipy: NaN)
 *   Everything after the sorted lists (vgan_outlier_score) is metric free.
 * vgan_outlier_knn_metric: vgan_outlier_knn for metric MANHATTAN, CHEBYSHEV or MINKOWSKI (any other is rejected: Euclidean
 *   and cosine lists come from vgan_outlier_knn) on the Minkowski-family producer (csrc/outlier_metric.hpp), a vector-ALU
 *   sweep with a 4 x 4 register tile per lane.  Pq / Pr are NOT centred packed blocks (vgan_outlier_pack with center NULL:
 *   a raw difference has one rounding).  The candidates are ranked by (g, index), g in float32 with the features ascending:
 *   the sum of |q_f - r_f|, their maximum, or the sum of exp2f(p log2f(|q_f - r_f|)) (no root: it is monotone).  Equal
 *   rows give g = 0 exactly.  For p > 2 a sum beyond FLT_MAX is +inf and such pairs compare equal (ranked by index); this is
 *   not guarded.  MINKOWSKI with p == 1 runs the MANHATTAN instance.  k, exclude_self, splits, part_d / part_i, nbr, the
 *   row-count and alignment rules and the independence of J and of the chunking are those of vgan_outlier_knn; all
 *   arguments are validated before the device is touched.
 * vgan_outlier_pack_unit: vgan_outlier_pack without a centre, every row divided by its float64 norm over F_s (the quotient
 *   rounded once to float32; a zero row stays zero); sq (may be NULL) [count, n] is exactly 1.0f for every row.  On these
 *   blocks vgan_outlier_knn with VGAN_OUTLIER_ENGINE_GRAM ranks by d2 = 2 - 2 cos, for every d_s, and a zero row lies at
 *   d2 = 2 (cosine distance 1) from every row without a special case in the sweep.
 * vgan_outlier_refine_metric: vgan_outlier_refine under `metric`: the k pairs re-measured in float64 from the raw rows
 *   (cosine: the dot product and both squared norms in float64, the distance clipped to [0, 2], exactly 1 when a norm is
 *   0), rounded to float32, re-sorted by (distance, index); kdist as there.  EUCLIDEAN, and MINKOWSKI with p == 2, run
 *   vgan_outlier_refine's kernel (the same bits); MINKOWSKI with p == 1 runs MANHATTAN.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_OUTLIER_MAX_K 32
#define VGAN_OUTLIER_METRIC_EUCLIDEAN 0
#define VGAN_OUTLIER_METRIC_MANHATTAN 1
#define VGAN_OUTLIER_METRIC_CHEBYSHEV 2
#define VGAN_OUTLIER_METRIC_MINKOWSKI 3
#define VGAN_OUTLIER_METRIC_COSINE 4
#define VGAN_OUTLIER_MAX_P 8.0
#define VGAN_OUTLIER_ENGINE_EXACT 0
#define VGAN_OUTLIER_ENGINE_GRAM 1
#define VGAN_OUTLIER_KNN_LARGEST 0
#define VGAN_OUTLIER_KNN_MEAN 1
#define VGAN_OUTLIER_KNN_MEDIAN 2
#define VGAN_OUTLIER_LRD 3
#define VGAN_OUTLIER_LOF 4
#define VGAN_OUTLIER_KDE_MAX_ROWS 8388607 /* 2^23 - 1 */
int vgan_outlier_pack(const float* X, int ldx, int n, int d, const float* center, const int32_t* feat,
                      const int32_t* feat_off, const int64_t* col_off, int first, int count, float* packed, float* sq,
                      vgan_stream_t stream);
int vgan_outlier_knn(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                     const int32_t* feat_off, const int64_t* col_off, int first, int count, int k, int exclude_self,
                     int engine, int splits, float* part_d, int32_t* part_i, int32_t* nbr, vgan_stream_t stream);
int vgan_outlier_refine(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                        const int32_t* feat_off, int first, int count, const int32_t* nbr, int k, int32_t* out_idx,
                        float* out_dist, float* kdist, vgan_stream_t stream);
int vgan_outlier_pack_unit(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off,
                           const int64_t* col_off, int first, int count, float* packed, float* sq, vgan_stream_t stream);
int vgan_outlier_knn_metric(const float* Pq, int nq, const float* Pr, int nr, const int32_t* feat_off, const int64_t* col_off,
                            int first, int count, int k, int exclude_self, int metric, double p, int splits, float* part_d,
                            int32_t* part_i, int32_t* nbr, vgan_stream_t stream);
int vgan_outlier_refine_metric(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                               const int32_t* feat_off, int first, int count, const int32_t* nbr, int k, int metric, double p,
                               int32_t* out_idx, float* out_dist, float* kdist, vgan_stream_t stream);
int vgan_outlier_score(const int32_t* idx, const float* dist, int nq, int k, int count, int method, const float* kdist_ref,
                       const double* lrd_ref, int nr, float* score, const int32_t* score_row, int ld_score, double* lrd_out,
                       vgan_stream_t stream);
int vgan_outlier_kde(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                     const int32_t* feat_off, const int64_t* col_off, int first, int count, const double* bandwidth,
                     int exclude_self, int engine, int splits, uint32_t* pivot, uint64_t* acc, float* score,
                     const int32_t* score_row, int ld_score, vgan_stream_t stream);
int vgan_outlier_combine(const float* score, int ld, int S, int n, const double* weights, double* out,
                         vgan_stream_t stream);
int vgan_outlier_abod(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                      const int32_t* feat_off, int first, int count, const int32_t* idx, int k, float* score,
                      const int32_t* score_row, int ld_score, vgan_stream_t stream);
int vgan_outlier_abod_floor(float* score, int ld, int S, int n, int fit, double* score_floor, int32_t* n_degenerate,
                            vgan_stream_t stream);
#define VGAN_OUTLIER_COF_CHAIN_SBN 0
#define VGAN_OUTLIER_COF_CHAIN_RANK 1
int vgan_outlier_cof_chain(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                           const int32_t* feat_off, int first, int count, const int32_t* idx, int k, int chain,
                           double* ac_out, vgan_stream_t stream);
int vgan_outlier_cof_score(const double* ac_q, int nq, const double* ac_ref, int nr, const int32_t* idx, int k, int count,
                           float* score, const int32_t* score_row, int ld_score, vgan_stream_t stream);
int vgan_outlier_cof_ceiling(float* score, int ld, int S, int n, int fit, double* score_ceiling, int32_t* n_degenerate,
                             vgan_stream_t stream);
#define VGAN_OUTLIER_NORM_ZSCORE 1
#define VGAN_OUTLIER_NORM_ROBUST 2
#define VGAN_OUTLIER_NORM_MINMAX 3
#define VGAN_OUTLIER_COMBINE_SUM 0
#define VGAN_OUTLIER_COMBINE_MAX 1
int64_t vgan_outlier_score_stats_ws_bytes(int S, int n, int mode);
int vgan_outlier_score_stats(const float* score, int ld, int S, int n, int mode, double* center, double* scale,
                             void* workspace, int64_t workspace_bytes, vgan_stream_t stream);
int vgan_outlier_combine_normalized(const float* score, int ld, int S, int n, const double* center, const double* scale,
                                    const double* weights, int combination, double* out, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Batched k-means over the subspaces of a SUBSPACE TABLE and the cluster-based local outlier factor (CBLOF; He, Xu,
 * Deng 2003; pyod's CBLOF) on top of it  (v-gan_amd/outlier.py: SubspaceCBLOF).  C = n_clusters, 2 <= C <=
 * VGAN_CLUSTER_MAX_CLUSTERS, squared Euclidean distance over the raw features of each subspace.  Per-subspace state
 * lives in device arrays indexed by table position s:
 *   centers   float64, the [C, d_s] centres of subspace s at element C * feat_off[s]: the master copy;
 *   changed   int32 [S], labels changed by the last E step (cleared by the M step); done int32 [S], 0 running,
 *             1 an E step changed no label (strict convergence), 2 the tolerance rule; n_iter int32 [S], M steps done;
 *   tol_var   float64 [S]: an M step whose summed squared centre shift is <= tol_var[s] ends the subspace; 0 disables.
 * and per chunk: img float32, the centres as the distance engines read them (chunk subspace s: [C, w_s] at element
 * C * (col_off[s] - col_off[first]), minus col_center[feat] when col_center is given, zero padded), img_sq [count, C]
 * its squared row norms (Gram engine), label int32 [count, n] (the caller fills it with -1 before the first iteration).
 * vgan_cluster_image: img / img_sq (may be NULL) from centers, for the chunk.
 * vgan_cluster_lloyd: enqueues `iterations` Lloyd iterations for the chunk; nothing is read back.  One iteration:
 *   E  every row of the packed block Pq (sq_q: its norms, Gram engine; as for vgan_outlier_knn) takes the centre with the
 *      smallest (engine d2, centre index); changed[s] counts the labels that differ from the previous ones;
 *   M  changed[s] == 0: done[s] = 1 and no M step.  Otherwise every centre becomes the float64 mean of its raw rows
 *      X [n, d] (ldx), summed over a fixed partition of the rows (slices of VGAN_CLUSTER_SLICE_ROWS rows by
 *      n, inside a slice row groups by C and d_s, then the slices in order; never by the chunk): no float atomics, the
 *      same bits for every chunking.  A
 *      cluster without rows keeps its centre.  img / img_sq are rewritten, n_iter[s] += 1, the tolerance rule is applied.
 *   A subspace with done[s] != 0 is skipped by every kernel.  total_dims = sum of d_s over the chunk, max_dims = the
 *   largest d_s; workspace: 16-byte aligned, vgan_cluster_lloyd_ws_bytes(n, C, count, total_dims) bytes (-1 for bad
 *   arguments).  n >= C.
 * vgan_cluster_final: float64 from the raw rows Xq [nq, d] (ldq) and centers, all S subspaces of the table.
 *   large == NULL  label [S, nq] = the nearest centre by (d2, index); sizes int64 [S, C] += the label counts (zeroed by
 *                  the caller); inertia [S] = sum of the d2 to the own centre (inertia_part: float64 workspace
 *                  [S, ceil(nq / 64)]; fixed order).
 *   large != NULL  (int32 [S, C], non-zero: a large cluster) score[row, q] = the distance to the own centre if it is
 *                  large, otherwise to the nearest large centre, times sizes[s, label] if use_weights (float32; row =
 *                  score_row[s], or s when score_row is NULL; ld_score >= nq); label may be NULL.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_CLUSTER_MAX_CLUSTERS 64
#define VGAN_CLUSTER_SLICE_ROWS 1024
int64_t vgan_cluster_lloyd_ws_bytes(int n, int n_clusters, int count, int total_dims);
int vgan_cluster_image(const double* centers, int n_clusters, const int32_t* feat, const int32_t* feat_off,
                       const int64_t* col_off, int first, int count, const float* col_center, float* img, float* img_sq,
                       vgan_stream_t stream);
int vgan_cluster_lloyd(const float* Pq, const float* sq_q, const float* X, int ldx, int n, int d, const int32_t* feat,
                       const int32_t* feat_off, const int64_t* col_off, int first, int count, int total_dims, int max_dims,
                       int n_clusters, int engine, const float* col_center, const double* tol_var, double* centers,
                       float* img, float* img_sq, int32_t* label, int32_t* changed, int32_t* done, int32_t* n_iter,
                       void* workspace, int64_t workspace_bytes, int iterations, vgan_stream_t stream);
int vgan_cluster_final(const float* Xq, int ldq, int nq, int d, const int32_t* feat, const int32_t* feat_off, int S,
                       int n_clusters, const double* centers, const int32_t* large, int64_t* sizes, int use_weights,
                       int32_t* label, double* inertia_part, double* inertia, float* score, const int32_t* score_row,
                       int ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ECOD (Li, Zhao, Hu, Botta, Ionescu, Chen 2022; pyod's ECOD): empirical-CDF tail probabilities per feature, summed over
 * the features of each subspace  (v-gan_amd/outlier.py: SubspaceECOD; kernels in csrc/outlier_ecod.hip).  All arithmetic
 * is float64 on the float32 data; -0.0 counts as +0.0 everywhere.  n is the number of rows given to fit, 1 <= n <=
 * VGAN_ECOD_MAX_ROWS.
 * vgan_ecod_sort_columns: sorted [d, n_pad] float32 receives every column of X [n, d] (ldx) in ascending order, column f
 *   at element f * n_pad; n_pad is the power of two with n <= n_pad < 2 n, and the entries past n are +inf.  A bitonic
 *   network on orderable integer keys (runs of VGAN_ECOD_SORT_RUN keys in LDS, one launch per longer stride), in place in
 *   `sorted`: no workspace.  The result is the unique ascending column (numpy.sort bit for bit once -0.0 is +0.0); the
 *   network is data independent, so NaN input changes no trip count (a NaN sorts above or below every number by its sign).
 * vgan_ecod_skew_sign: sign int8 [d] = the sign of the skewness of each column of a column-major image [d, ld] (n entries
 *   a column; the sorted image serves): mu = sum(x) / n, m2 = sum((x - mu)^2), m3 = sum((x - mu)^3), two passes in a
 *   fixed order; sign = 0 if m2 == 0, else -1 / 0 / +1 by m3.  The same bits from run to run.
 * vgan_ecod_tail_counts: for the query rows Xq [rows, d] (ldq): cl [rows, d] = #{r : X[r, f] <= x} and cr [rows, d] =
 *   #{r : X[r, f] >= x} (int32; upper_bound and n - lower_bound in the sorted column), by binary searches of a fixed
 *   number of steps.  The counts are those among the n fitted rows: a new row is NOT counted (vgan_ecod_scores adds it).
 * vgan_ecod_scores: from the counts, per (row, feature): ul = -log((cl + a) / (n + a)), ur = -log((cr + a) / (n + a)), a = 0
 *   for query == 0 (fit: the row is among the n) and 1 otherwise (the row scored alone, appended to the n); the quotient
 *   is one IEEE division, then log.  usk = ul if sign[f] < 0, ur if sign[f] > 0, ul + ur if sign[f] == 0.  With mask
 *   float64 [d, ldm] (mask[f, s] = 1 if feature f belongs to subspace s, else 0; ldm >= S):
 *     VGAN_ECOD_AGGREGATE_DIMENSION  score[s, i] = sum_f mask[f, s] max(ul, ur, usk)                      (pyod's code)
 *     VGAN_ECOD_AGGREGATE_TAIL       score[s, i] = max(sum_f mask ul, sum_f mask ur, sum_f mask usk)       (the paper)
 *   in float64 on the f64 matrix unit, f ascending, rounded to float32 into score [S, ld_score] (ld_score >= rows).
 *   terms: float64 workspace of rows * d (DIMENSION) or 3 * rows * d (TAIL) elements.  The bits of score[s, i] depend on
 *   the row's counts alone, not on its position in the call: any split of the rows over calls gives the same matrix.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_ECOD_SORT_RUN 2048
#define VGAN_ECOD_MAX_ROWS 16777216 /* 2^24 */
#define VGAN_ECOD_AGGREGATE_DIMENSION 0
#define VGAN_ECOD_AGGREGATE_TAIL 1
int vgan_ecod_sort_columns(const float* X, int ldx, int n, int d, float* sorted, int64_t n_pad, vgan_stream_t stream);
int vgan_ecod_skew_sign(const float* sorted, int64_t ld, int n, int d, int8_t* sign, vgan_stream_t stream);
int vgan_ecod_tail_counts(const float* Xq, int ldq, int rows, int d, const float* sorted, int64_t ld, int n, int32_t* cl,
                          int32_t* cr, vgan_stream_t stream);
int vgan_ecod_scores(const int32_t* cl, const int32_t* cr, int rows, int d, const int8_t* sign, int n, int query,
                     int aggregate, const double* mask, int ldm, int S, double* terms, float* score, int64_t ld_score,
                     vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Histogram outlier scores: HBOS (Goldstein and Dengel 2012; pyod's HBOS) and LODA (Pevny 2016; pyod's LODA) over the
 * subspaces  (v-gan_amd/outlier.py: SubspaceHBOS and SubspaceLODA, whose docstrings are the definitions; kernels in
 * csrc/outlier_hist.hip).  They replace numpy.histogram per feature (HBOS) and per random projection (LODA) and the
 * numpy.digitize / searchsorted lookups of pyod's scoring.  A COLUMN is a feature of X (HBOS: P = d) or the projected value
 * of one projection of one subspace (LODA: P = S k, column s k + j).  All arithmetic is float64 on the float32 data; -0.0
 * counts as +0.0.  2 <= B <= VGAN_HIST_MAX_BINS bins; at most VGAN_HIST_MAX_ROWS rows a call.
 * keys uint64 [P, 2]: order-preserving integer keys of a column's float64 minimum and maximum, gathered with integer
 *   atomics (exact in any order).  edges float64 [P, B + 1]; counts int32 [P, B].
 * vgan_hist_column_range: keys of the d columns of X [n, d] (ldx); sets them first.
 * vgan_hist_edges: lo, hi from the keys (lo == hi: lo - 0.5, lo + 0.5, numpy.histogram's rule), step = (hi - lo) / B,
 *   e_j = j * step + lo in two roundings, e_B = hi: numpy.linspace(lo, hi, B + 1) bit for bit.
 * vgan_hist_column_counts: counts of the d columns of X: the bin of x is #{j in 1 .. B - 1 : e_j <= x} (numpy.histogram's;
 *   a value outside [lo, hi] falls into the first or last bin), by a search of a fixed number of steps; LDS integer
 *   histograms flushed with integer atomics.  Zeroes counts first.
 * vgan_hbos_scores: for the query rows Xq [rows, d] (ldq): T[i, f] = table[f, bin(x)], or table[f, B] where x <
 *   limits[f, 0] or x > limits[f, 1]; table float64 [d, B + 1] (term_f[0 .. B - 1], then the out-of-range term) and limits
 *   float64 [d, 2] are built on the host from the counts (hbos_term_table).  Then score[s, i] = sum_f mask[f, s] T[i, f]
 *   on the f64 matrix unit, f ascending, rounded to float32 into score [S, ld_score]: the product of vgan_ecod_scores.
 *   terms: float64 workspace of rows * d elements.  The bits of score[s, i] depend on the row alone.
 * vgan_hist_reset: keys (may be NULL) to (above every key, below every key), counts (may be NULL) to 0: before the first
 *   of the vgan_loda_range / vgan_loda_counts calls that accumulate into them over row chunks.
 * vgan_loda_*: P is the PACKED block (vgan_outlier_pack, not centred) of `rows` rows for the subspaces first .. first + count
 *   - 1 of the table (count <= 65535; max_dims >= every round4(d_s) of the range, at most VGAN_LODA_MAX_DIMS).  Subspace s
 *   has k projections of m_s = moff[s + 1] - moff[s] nonzeros each (moff int64 [S + 1]); nonzero t of projection j is
 *   pidx / pw [k * moff[s] + t * k + j]: a position within the subspace (clamped to it) and a float64 weight.  z = (((0 + w_0
 *   x_0) + w_1 x_1) + ...), every product and sum rounded on its own.  1 <= k <= VGAN_LODA_MAX_PROJECTIONS.
 *   vgan_loda_range merges the keys of z over the rows into keys [S k, 2]; vgan_loda_counts adds the bins of z to counts
 *   [S k, B]; vgan_loda_scores writes score[s, i] = float32((1 / k) sum_j terms[s k + j, bin(z_j)]) into score [S, ld_score]
 *   (terms float64 [S k, B], built on the host: loda_term_table), the sum in an order fixed by k alone.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_HIST_MAX_BINS 256
#define VGAN_HIST_MAX_ROWS 16777216 /* 2^24: the counts stay in int32 */
#define VGAN_LODA_MAX_PROJECTIONS 1024
#define VGAN_LODA_MAX_DIMS 8192 /* packed features of one subspace: a row of it is staged in LDS */
int vgan_hist_column_range(const float* X, int ldx, int n, int d, uint64_t* keys, vgan_stream_t stream);
int vgan_hist_edges(const uint64_t* keys, int64_t P, int B, double* edges, vgan_stream_t stream);
int vgan_hist_column_counts(const float* X, int ldx, int n, int d, const double* edges, int B, int32_t* counts,
                            vgan_stream_t stream);
int vgan_hbos_scores(const float* Xq, int ldq, int rows, int d, const double* edges, int B, const double* table,
                     const double* limits, const double* mask, int ldm, int S, double* terms, float* score, int64_t ld_score,
                     vgan_stream_t stream);
int vgan_hist_reset(uint64_t* keys, int64_t P, int32_t* counts, int64_t cells, vgan_stream_t stream);
int vgan_loda_range(const float* P, int rows, const int32_t* feat_off, const int64_t* col_off, int first, int count,
                    int max_dims, const int32_t* pidx, const double* pw, const int64_t* moff, int k, uint64_t* keys,
                    vgan_stream_t stream);
int vgan_loda_counts(const float* P, int rows, const int32_t* feat_off, const int64_t* col_off, int first, int count,
                     int max_dims, const int32_t* pidx, const double* pw, const int64_t* moff, int k, const double* edges,
                     int B, int32_t* counts, vgan_stream_t stream);
int vgan_loda_scores(const float* P, int rows, const int32_t* feat_off, const int64_t* col_off, int first, int count,
                     int max_dims, const int32_t* pidx, const double* pw, const int64_t* moff, int k, const double* edges,
                     int B, const double* terms, float* score, int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Isolation forest (Liu, Ting, Zhou 2008; sklearn's IsolationForest, pyod's IForest): T random trees per subspace on psi
 * sampled rows each; a row's score falls with its mean path length  (v-gan_amd/outlier.py: SubspaceIForest, whose docstring
 * is the definition; kernels in csrc/outlier_iforest.hip).  L = ceil(log2 psi) is the depth limit, N = 2^(L + 1) the slots
 * of a heap-numbered tree (root 1, children 2 i and 2 i + 1, slot 0 unused).  nodes is int32 [S, T, N, 2]: word 0 the split
 * feature (a column of X; -1 a leaf, -2 an absent slot), word 1 the float32 threshold of an internal node (a row goes left
 * iff x <= threshold), the sample rows of a leaf, 0 where absent.  2 <= psi <= VGAN_IFOREST_MAX_SAMPLES, 1 <= T <=
 * VGAN_IFOREST_MAX_TREES; the three entries take the same (T, psi, L) and reject an L that is not ceil(log2 psi).
 * vgan_iforest_build: the T trees of the subspaces first .. first + count - 1 of the table (feat, feat_off: the feature
 *   lists, concatenated, and their offsets) from X [n, d] (ldx), 2 <= psi <= n <= 2^31 - 1, into their slots of nodes.
 *   Tree (s, t) has the stream id = s T + t: its sample is rows feistel_perm(i, n, seed, id), i < psi (the permutation of
 *   vgan_shuffle_index); a node of m rows at depth e is a leaf if m <= 1, e == L or no feature of the subspace varies on its
 *   rows (float32 min == max, -0.0 as +0.0); otherwise the Philox4x32-10 words (w0, w1, ., .) of counter (node, 0,
 *   0x49464F52, 0) and key (lo32(seed) ^ lo32(id), hi32(seed) ^ hi32(id) ^ 0x5bd1e995) choose the j-th varying feature in
 *   ascending feature order, j = (w0 c) >> 32 for c varying features, and the threshold p = float32(lo + u (hi - lo)) with
 *   u = (w1 + 0.5) 2^-32 and lo, hi the feature's min and max on the rows, in three separately rounded float64 operations;
 *   p >= hi is replaced by lo.  One workgroup per tree, the rows in LDS; no workspace.  max_dims: no subspace of the range
 *   has more features (at most VGAN_IFOREST_MAX_DIMS).  The trees depend on the row sets alone: the same bits from run
 *   to run and for every split of the subspaces over calls.
 * vgan_iforest_path_sums: sums int64 [count, ld_sums] (ld_sums >= rows): for every query row of Xq [rows, d] (ldq) and every
 *   subspace of the range the total over its T trees of (e << 32) + cq[m], e the depth and m the size of the leaf the row
 *   reaches; cq int64 [psi + 1] is the Q32 image of the average path length c(m), formed on the host (the device computes no
 *   logarithm).  Integer sums: the same for every split of the rows or the subspaces over calls.  count <= 65535.
 * vgan_iforest_scores: score float32 [count, ld_score] = float32(exp2(-(double(sum) / double(denom)))), denom = T cq[psi] > 0.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_IFOREST_MAX_SAMPLES 1024
#define VGAN_IFOREST_MAX_TREES 1024
#define VGAN_IFOREST_MAX_DIMS 8192
int vgan_iforest_build(const float* X, int ldx, int64_t n, int d, const int32_t* feat, const int32_t* feat_off, int first,
                       int count, int max_dims, int T, int psi, int L, uint64_t seed, int32_t* nodes, vgan_stream_t stream);
int vgan_iforest_path_sums(const float* Xq, int ldq, int rows, int d, const int32_t* nodes, int first, int count, int T,
                           int psi, int L, const int64_t* cq, int64_t* sums, int64_t ld_sums, vgan_stream_t stream);
int vgan_iforest_scores(const int64_t* sums, int64_t ld_sums, int count, int rows, int64_t denom, float* score,
                        int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Oblique cuts for the isolation forest (the extended isolation forest of Hariri, Carrasco Kind and Brunner, TKDE 2019;
 * SCiForest, Liu, Ting, Zhou 2010): every internal node cuts with a random sparse hyperplane over at most q of the
 * subspace's features, 2 <= q <= VGAN_IFOREST_MAX_PLANE  (SubspaceIForest(n_dims = q), whose docstring is the definition:
 * candidates, attempts, positions, weights, projection, threshold; kernels in csrc/outlier_iforest.hip).  Trees, samples,
 * stream ids, heap numbering, L, N, cq and vgan_iforest_scores are those of the section above.  Both entries take DENSE
 * row-major matrices: row i starts i d floats after the base, there is no leading dimension.
 * nodes is int32 [S, T, N, 2]: word 0 the successful attempt (0 .. 3) of an internal node, -1 a leaf, -2 an absent slot;
 * word 1 the float32 threshold of an internal node (a row goes left iff float32(projection) <= threshold), the sample rows
 * of a leaf, 0 where absent.  plane_col int32 [S, T, N, q]: the columns of X of the slot's hyperplane, ascending, -1 in the
 * unused places and everywhere outside internal nodes; plane_w float32 [S, T, N, q]: their weights, 0 where unused.
 * vgan_iforest_build_oblique: the T trees of the subspaces first .. first + count - 1 from X [n, d], 2 <= psi <= n <= 2^31 -
 *   1; cand: the candidate features (columns of X, ascending per subspace) of all subspaces, concatenated, cand_off int32
 *   [S + 1] their offsets; a subspace without candidates gets root leaves.  The attempts a = 0 .. 3 of a node use the
 *   Philox4x32-10 blocks at counter (node, 32 a + b, 0x45494600, 0) under the tree's key: b = 0 the threshold word, 1 .. 4
 *   the positions, 5 + i weight i.  One workgroup per tree; a node reads only its own at most q features.  count <= 65535.
 * vgan_iforest_path_sums_oblique: vgan_iforest_path_sums on such trees, Xq [rows, d] dense; sums int64 [count, ld_sums],
 *   ld_sums >= rows.  A plane is read up to its first entry outside [0, d): no column outside Xq is ever read, whatever the
 *   planes hold.
 * Both return VGAN_ERR_ARG before touching the device when an argument is out of range (null pointers, n < psi, psi, T, L,
 * q, count, ld_sums).
 * ------------------------------------------------------------------------------------------- */
#define VGAN_IFOREST_MAX_PLANE 16
int vgan_iforest_build_oblique(const float* X, int64_t n, int d, const int32_t* cand, const int32_t* cand_off, int first,
                               int count, int T, int psi, int L, int q, uint64_t seed, int32_t* nodes, int32_t* plane_col,
                               float* plane_w, vgan_stream_t stream);
int vgan_iforest_path_sums_oblique(const float* Xq, int rows, int d, const int32_t* nodes, const int32_t* plane_col,
                                   const float* plane_w, int first, int count, int T, int psi, int L, int q, const int64_t* cq,
                                   int64_t* sums, int64_t ld_sums, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * RS-Hash (Sathe and Aggarwal, ICDM 2016): T components per subspace, each a randomly shifted grid of width f over r of the
 * subspace's non-constant features, holding how many of s sampled rows fall into each occupied cell; a row's score falls
 * with the log of the count of its own cell  (v-gan_amd/outlier.py: SubspaceRSHash, whose docstring is the definition;
 * kernels in csrc/outlier_rshash.hip).  2 <= s <= VGAN_RSHASH_MAX_SAMPLES, 1 <= T <= VGAN_RSHASH_MAX_COMPONENTS; the three
 * entries take the same (T, s).  COMPONENT c = z T + t is component t of subspace z; the host draws its parameters
 * (rshash_components): comp_dims int32 [S, T] (r, 0 .. VGAN_RSHASH_MAX_DIMS; 0: the subspace has no candidate feature),
 * comp_feat int32 [S, T, VGAN_RSHASH_MAX_DIMS] (columns of X, ascending; held to [0, d)), comp_shift float64 [S, T,
 * VGAN_RSHASH_MAX_DIMS] (alpha) and comp_width float64 [S, T] (f, in [1 / 64, 63 / 64]).
 * The digit of a value x of chosen feature j: x' = (x - mn_j) / w_j, 0 where w_j = mx_j - mn_j is 0; y = floor((x' + alpha_j)
 *   / f) clamped to [-1, floor(1 / f) + 2] (NaN to -1); digit = y + 1.  Float64 on the float32 values, every operation
 *   rounded on its own.  R = floor(1 / f) + 4 and key = sum_j digit_j R^j in uint64, j over the chosen features in order.
 * vgan_rshash_build: the components of the subspaces first .. first + count - 1 from X [n, d] (ldx), s <= n <=
 *   VGAN_RSHASH_MAX_ROWS.  The sample of component c is rows feistel_perm(i, n, seed, c), i < s (the permutation of
 *   vgan_shuffle_index).  sample_min / sample_max float32 [S, T, VGAN_RSHASH_MAX_DIMS]: the exact float32 min and max of
 *   every chosen feature over the sample, -0.0 as +0.0, 0 past r.  cell_key uint64 [S, T, s]: the distinct keys of the
 *   sampled rows, ascending, then 2^64 - 1; cell_count int32 [S, T, s]: their counts, then 0; n_cells int32 [S, T].  r = 0:
 *   no cell.  sample_rows int32 [S, T, s] (may be NULL) receives the sample's row indices, ascending.  One workgroup per
 *   component, sample and keys in LDS; no workspace.  Everything depends on the row sets alone: the same bits from run to
 *   run and for every split of the subspaces over calls.
 * vgan_rshash_cell_sums: sums int64 [count, ld_sums] (ld_sums >= rows): for every query row and every subspace of the range
 *   the total over its T components of table[c_t]: c_t the count of the cell of the row's key (0 where absent), plus 1 --
 *   except, when sample_rows is given (the fit), for a row that is in the component's sample: row i of the call is row
 *   row_base + i of the fitted X.  A component with r = 0 adds table[s + 1].  table int64 [s + 2] is formed on the host
 *   (rshash_log_table: rint(log2(c) 2^32); the device computes no logarithm).  Element (i, f) of the query rows is
 *   Xq[i row_stride + f col_stride]: row-major (col_stride 1, row_stride >= d) or column-major (row_stride 1, col_stride
 *   >= rows).  Integer sums: the same for every split of the rows or the subspaces over calls.  count <= 65535.
 * vgan_rshash_scores: score float32 [count, ld_score] = float32(1 - double(sum) / double(denom)), denom = T table[s + 1] > 0.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_RSHASH_MAX_SAMPLES 4096 /* the sample's row indices and keys live in LDS */
#define VGAN_RSHASH_MAX_COMPONENTS 1024
#define VGAN_RSHASH_MAX_DIMS 12 /* r at s = 4096 */
#define VGAN_RSHASH_MAX_ROWS 16777216 /* 2^24: the range pass of the candidate features */
int vgan_rshash_build(const float* X, int ldx, int64_t n, int d, int first, int count, int T, int s, uint64_t seed,
                      const int32_t* comp_dims, const int32_t* comp_feat, const double* comp_shift, const double* comp_width,
                      uint64_t* cell_key, int32_t* cell_count, int32_t* n_cells, float* sample_min, float* sample_max,
                      int32_t* sample_rows, vgan_stream_t stream);
int vgan_rshash_cell_sums(const float* Xq, int64_t row_stride, int64_t col_stride, int rows, int d, int64_t row_base, int first,
                          int count, int T, int s, const int32_t* comp_dims, const int32_t* comp_feat, const double* comp_shift,
                          const double* comp_width, const uint64_t* cell_key, const int32_t* cell_count, const int32_t* n_cells,
                          const float* sample_min, const float* sample_max, const int32_t* sample_rows, const int64_t* table,
                          int64_t* sums, int64_t ld_sums, vgan_stream_t stream);
int vgan_rshash_scores(const int64_t* sums, int64_t ld_sums, int count, int rows, int64_t denom, float* score,
                       int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Deep isolation forest (Xu, Pang, Wang, Wang, TKDE 2023; pyod's DIF): r randomly initialised, never trained MLPs per
 * subspace map its rows to representations of q columns, and T isolation trees are grown on every representation
 * (v-gan_amd/outlier.py: SubspaceDIF, whose docstring is the definition; kernels in csrc/outlier_dif.hip and, for the trees,
 * csrc/outlier_iforest.hip).  BLOCK b = s r + j is representation j of subspace s of the table (feat, feat_off).  Its net has
 * the layer sizes K_0 = d_s = feat_off[s + 1] - feat_off[s], hidden[0 .. n_hidden - 1], q; no bias; the activation after every
 * layer but the last.  Limits: 1 <= r <= VGAN_DIF_MAX_NETS, 0 <= n_hidden <= VGAN_DIF_MAX_HIDDEN (hidden is a HOST array, NULL
 * only when n_hidden is 0), 1 <= hidden[l] <= VGAN_DIF_MAX_WIDTH, 1 <= q <= VGAN_DIF_MAX_OUT, count <= 65535 blocks a call.
 * The weights of the blocks first .. first + count - 1 live in one float32 buffer W (16-byte aligned): block first + z starts at
 *   W + w_off[z] (w_off int64 [count] on the device, multiples of 8), its layers follow one another, layer l stored
 *   quad-major as [ld_l / 4][K_{l+1}][4] with ld_l = K_l rounded up to 8: W_l[o, i] at ((i >> 2) K_{l+1} + o) 4 + (i & 3), and
 *   FINITE values (vgan_dif_weights writes zeros) in the pad positions i >= K_l.
 * vgan_dif_weights: zeroes W[0 .. total) and writes W_l[o, i] = float32((2 u - 1) c_l) of every block of the range: u = (w + 0.5)
 *   2^-32 in float64, w the word e & 3, e = o K_l + i, of Philox4x32-10 at counter (lo32(e >> 2), hi32(e >> 2), 0x44494600 + l, 0)
 *   and key (lo32(seed) ^ lo32(b), hi32(seed) ^ hi32(b) ^ 0x5bd1e995), b the absolute block; c_l = scale[s (n_hidden + 1) + l]
 *   (float64 on the device, formed on the host as 1 / sqrt(K_l): the device computes no square root).
 * vgan_dif_represent: R float32 [count, rows, q]: the net of every block of the range applied to z restricted to the features
 *   of its subspace, z = float32((double(x) - double(lo_f)) / (double(hi_f) - double(lo_f))), 0 where hi_f == lo_f (lo, hi
 *   float32 [d]), read from X [rows, d] (ldx) through the feature list; rows <= VGAN_DIF_MAX_ROWS.  Products accumulate in
 *   float32 on the fp32-input matrix unit, every element one chain over k in an order fixed by k alone; tanh is
 *   float32(tanh(double(a))), relu max(a, 0).  One workgroup per (block, VGAN_DIF_ROW_TILE rows); layer 0 is staged
 *   VGAN_DIF_K_TILE features at a time, the later activations stay in LDS.  An element of R depends on its row, block and
 *   column alone: the same bits for every split of the rows or blocks over calls.
 * vgan_iforest_build_blocks / vgan_iforest_path_sums_blocks: vgan_iforest_build / vgan_iforest_path_sums with one matrix PER
 *   BLOCK instead of one feature list per subspace: block first + z reads R + z block_stride as [n, q] (rows of q floats;
 *   block_stride >= n q), every column a candidate, the stored split feature a column 0 .. q - 1; nodes is int32 [blocks, T, N, 2]
 *   indexed by the ABSOLUTE block, and tree (b, t) has the stream id b T + t.  sums int64 [count, ld_sums].  Same rules, same
 *   kernels and the same (T, psi, L) checks as the subspace entries.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_DIF_MAX_NETS 256
#define VGAN_DIF_MAX_HIDDEN 3
#define VGAN_DIF_MAX_WIDTH 512
#define VGAN_DIF_MAX_OUT 64
#define VGAN_DIF_MAX_ROWS 16777216 /* 2^24 */
#define VGAN_DIF_ROW_TILE 32
#define VGAN_DIF_K_TILE 64
#define VGAN_DIF_ACT_TANH 0
#define VGAN_DIF_ACT_RELU 1
int vgan_dif_weights(const int32_t* feat_off, int r, int first, int count, int n_hidden, const int32_t* hidden, int q,
                     const double* scale, uint64_t seed, float* W, const int64_t* w_off, int64_t total, vgan_stream_t stream);
int vgan_dif_represent(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const float* lo,
                       const float* hi, int r, int first, int count, int n_hidden, const int32_t* hidden, int q, int activation,
                       const float* W, const int64_t* w_off, float* R, vgan_stream_t stream);
int vgan_iforest_build_blocks(const float* R, int64_t block_stride, int64_t n, int q, int first, int count, int T, int psi, int L,
                              uint64_t seed, int32_t* nodes, vgan_stream_t stream);
int vgan_iforest_path_sums_blocks(const float* Rq, int64_t block_stride, int rows, int q, const int32_t* nodes, int first,
                                  int count, int T, int psi, int L, const int64_t* cq, int64_t* sums, int64_t ld_sums,
                                  vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Autoencoder outlier scores (pyod's AutoEncoder without dropout and batch normalisation; replaces a host framework's loop of
 * nn.Linear forward / MSELoss backward / torch.optim.Adam(weight_decay=) steps over S small nets): one MLP per subspace of the
 * table (feat, feat_off), trained to reconstruct the standardised rows, scored by the reconstruction distance
 * (v-gan_amd/outlier.py: SubspaceAutoEncoder, whose docstring is the definition; kernels in csrc/outlier_ae.hip).  BLOCK b is
 * the subspace at position b.  Its net has the layer sizes K_0 = d_s, hidden[0 .. n_hidden - 1], hidden[n_hidden - 2 .. 0],
 * d_s (2 n_hidden layers), a bias in every layer, the activation after every layer but the last.  Limits: 1 <= n_hidden <=
 * VGAN_AE_MAX_HIDDEN (hidden is a HOST array), 1 <= hidden[l] <= VGAN_AE_MAX_WIDTH, d_s <= max_dims <= VGAN_AE_MAX_DIMS (a
 * block with more than max_dims features is left alone), count <= 65535 blocks a call.
 * The STATE of the blocks first .. first + count - 1 is one float32 buffer: block first + z starts at state + s_off[z] (s_off
 *   int64 [count] on the device) and holds theta, m and v, P = sum_l (K_l + 1) N_l floats each; inside each, layer after
 *   layer, W_l K-MAJOR [K_l][N_l] (W_l[o, i] at i N_l + o) followed by b_l [N_l].  vgan_ae_scores reads theta alone.
 * z = float32((double(x) - mean_f) / scale_f), mean and scale float64 [d] (scale 1 for a constant column).  skip int32 [S]:
 *   1 = the subspace is constant: it is not trained and scores exactly 0.
 * vgan_ae_init: zeroes state[0 .. total) and writes theta of every block of the range: W_l[o, i] and b_l[o] = float32((2 u - 1)
 *   c_l), u = (w + 0.5) 2^-32 in float64, w the word e & 3 of Philox4x32-10 at counter (lo32(e >> 2), hi32(e >> 2), 0x41450000 +
 *   l, 0) and key (lo32(seed) ^ lo32(b), hi32(seed) ^ hi32(b) ^ 0x5bd1e995), e = o K_l + i for a weight and N_l K_l + o for a
 *   bias; c_l = scale[b (2 n_hidden) + l] (float64 on the device, formed on the host as 1 / sqrt(K_l)).
 * vgan_ae_train: the global steps step_first .. step_first + step_count - 1 (0-based; step g is step g % (n / batch) of
 *   epoch g / (n / batch) and has t = g + 1) of every block of the range, ONE WORKGROUP PER BLOCK for the whole call.  Row j of
 *   the batch of step i of epoch e is feistel_perm(i batch + j, n, seed, e).  corr float64 [step_count, 2] on the device:
 *   1 - beta1^t and 1 - beta2^t of every step of the call, formed on the host.  Per step: z of the batch, the forward, the
 *   float32 loss sum (out - z)^2 / (batch d_s) into loss[z_block ld_loss + g] (before the update), the exact backward, g +=
 *   weight_decay theta, torch's Adam in place.  Every product is one fmaf chain in ascending order of its summation index,
 *   so the bits depend on neither the cut of the steps into calls nor the blocks that share a call.  The activations of the
 *   batch stay in LDS when batch (2 (max_dims | 1) + sum (h | 1) + (max h | 1)) <= VGAN_AE_LDS_FLOATS, the sum over the 2
 *   n_hidden - 1 hidden layers; otherwise scratch (float32, scratch_floats >= that many per block of the call) holds them.
 * vgan_ae_scores: score[z ld_score + i] = float32(sqrt(sum_f (out_if - z_if)^2)), the sum float64 in ascending f, for the rows
 *   of X [rows, d]; one workgroup per (block, VGAN_AE_ROW_TILE rows), the same layer routine as the training.  recon != NULL
 *   (count must be 1): float32 [rows, d_s] receives the raw output instead, score may be NULL.  scratch as above with
 *   VGAN_AE_ROW_TILE ((max_dims | 1) + sum (h | 1)) floats per (block, row tile).
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_AE_MAX_HIDDEN 3
#define VGAN_AE_MAX_WIDTH 128
#define VGAN_AE_MAX_DIMS 1024
#define VGAN_AE_MAX_BATCH 256
#define VGAN_AE_MAX_ROWS 16777216 /* 2^24 */
#define VGAN_AE_MAX_LAUNCH_STEPS 65536
#define VGAN_AE_ROW_TILE 32
#define VGAN_AE_LDS_FLOATS 38912 /* 152 KiB of the 160 KiB of a CU */
#define VGAN_AE_ACT_TANH 0
#define VGAN_AE_ACT_RELU 1
int vgan_ae_init(const int32_t* feat_off, int first, int count, int n_hidden, const int32_t* hidden, const double* scale,
                 uint64_t seed, float* state, const int64_t* s_off, int64_t total, vgan_stream_t stream);
int vgan_ae_train(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                  const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                  const int32_t* hidden, int activation, int batch, uint64_t seed, int64_t step_first, int step_count,
                  const double* corr, double lr, double beta1, double beta2, double eps, double weight_decay, float* state,
                  const int64_t* s_off, float* loss, int64_t ld_loss, float* scratch, int64_t scratch_floats,
                  vgan_stream_t stream);
int vgan_ae_scores(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                   const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                   const int32_t* hidden, int activation, const float* state, const int64_t* s_off, float* score,
                   int64_t ld_score, float* recon, float* scratch, int64_t scratch_floats, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Deep SVDD one-class scores (Ruff et al. 2018; pyod's DeepSVDD, the one-class objective): one encoder per subspace of the
 * table (feat, feat_off), trained to map the standardised rows onto one point c, scored by the squared distance of a row's
 * image from c (v-gan_amd/outlier.py: SubspaceDeepSVDD, whose docstring is the definition; kernels in csrc/outlier_svdd.hip,
 * the layer routines of csrc/outlier_mlp.hpp shared with the autoencoder).  BLOCK b is the subspace at position b.  Its net
 * has the layer sizes K_0 = d_s, hidden[0 .. n_hidden - 1] (n_hidden layers), NO BIAS, the activation after every layer but
 * the last; q = hidden[n_hidden - 1] <= VGAN_SVDD_MAX_OUT is the output dimension.  The limits, z, skip, the activations, the
 * batches, corr, Adam and the scratch rule are those of the vgan_ae_* entries (VGAN_AE_*).
 * The STATE of block first + z starts at state + s_off[z] and holds theta, m and v, P = sum_l K_l N_l floats each; inside
 *   each, layer after layer, W_l K-MAJOR [K_l][N_l] (W_l[o, i] at i N_l + o).
 * vgan_svdd_init: zeroes state[0 .. total) and writes theta: W_l[o, i] = float32((2 u - 1) c_l) by the rule of vgan_ae_init with
 *   the counter word 2 = VGAN_SVDD_PHILOX_TAG + l, e = o K_l + i; c_l = scale[b n_hidden + l].
 * vgan_svdd_center: the forward of the nets over the rows of X [rows, d], one workgroup per (block, VGAN_AE_ROW_TILE rows),
 *   which writes the float64 sum over its rows (ascending) of every output coordinate to tile_sums [count, tiles, q]
 *   (tile_cells >= count tiles q); then run_sums [count, q] (float64, zeroed by the caller before the first call) += the tile
 *   sums in tile order.  n_total = 0: more rows follow (every call but the last passes a multiple of VGAN_AE_ROW_TILE rows).
 *   n_total > 0, the last call: mean = run_sums / n_total; where center_eps > 0 and |mean| < center_eps the coordinate becomes
 *   -center_eps when mean < 0 and +center_eps otherwise; center [count, q] = float32 of it, n_clamped int32 [count] the number
 *   of coordinates the rule moved.  A block with skip = 1 gets a centre of zeros and n_clamped 0.
 * vgan_svdd_train: as vgan_ae_train with r = out - center[z_block], the float32 loss sum r^2 / batch into loss[z_block ld_loss +
 *   g] (before the update) and the output error r float32(2 / batch).  The activations of the batch stay in LDS when batch
 *   ((max_dims | 1) + sum (h | 1) + (max h | 1)) <= VGAN_AE_LDS_FLOATS; otherwise scratch holds them.
 * vgan_svdd_scores: score[z ld_score + i] = float32(sum_j double(out_ij - center_zj)^2), j ascending, the difference float32.
 *   embed != NULL (count must be 1): float32 [rows, q] receives the raw output instead; center and score may be NULL.
 *   scratch as above with VGAN_AE_ROW_TILE ((max_dims | 1) + sum (h | 1)) floats per (block, row tile).
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_SVDD_MAX_OUT 128 /* VGAN_AE_MAX_WIDTH */
#define VGAN_SVDD_PHILOX_TAG 1398162432 /* 0x53564400 */
int vgan_svdd_init(const int32_t* feat_off, int first, int count, int n_hidden, const int32_t* hidden, const double* scale,
                   uint64_t seed, float* state, const int64_t* s_off, int64_t total, vgan_stream_t stream);
int vgan_svdd_center(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                     const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                     const int32_t* hidden, int activation, const float* state, const int64_t* s_off, double* tile_sums,
                     int64_t tile_cells, double* run_sums, int64_t n_total, double center_eps, float* center,
                     int32_t* n_clamped, float* scratch, int64_t scratch_floats, vgan_stream_t stream);
int vgan_svdd_train(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                    const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                    const int32_t* hidden, int activation, int batch, uint64_t seed, int64_t step_first, int step_count,
                    const double* corr, double lr, double beta1, double beta2, double eps, double weight_decay,
                    const float* center, float* state, const int64_t* s_off, float* loss, int64_t ld_loss, float* scratch,
                    int64_t scratch_floats, vgan_stream_t stream);
int vgan_svdd_scores(const float* X, int ldx, int rows, int d, const int32_t* feat, const int32_t* feat_off, const double* mean,
                     const double* scale, const int32_t* skip, int first, int count, int max_dims, int n_hidden,
                     const int32_t* hidden, int activation, const float* state, const int64_t* s_off, const float* center,
                     float* score, int64_t ld_score, float* embed, float* scratch, int64_t scratch_floats,
                     vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * iNNE, isolation by nearest-neighbour ensembles (Bandaragoda, Ting, Albrecht, Liu, Wells 2018; pyod's INNE): T estimators
 * per subspace, each psi sampled rows (the centres) with a hypersphere around every centre that reaches its nearest other
 * centre; a row takes from an estimator the isolation ratio of the smallest sphere that covers it, 1 where none does
 * (v-gan_amd/outlier.py: SubspaceINNE, whose docstring is the definition; kernels in csrc/outlier_inne.hip).
 * 2 <= psi <= VGAN_INNE_MAX_SAMPLES, 1 <= T <= VGAN_INNE_MAX_ESTIMATORS.  The fitted state is four arrays [S, T, psi]:
 * rows int32 (the centres as rows of X, in draw order), r2 float64 (squared radii), nn int32 (the position of the nearest
 * other centre) and rho float64 (the isolation ratios); X itself stays with the caller and is read again at scoring.
 * d2(a, b): over the features of the subspace in ascending order, float64, acc = 0: diff = double(a_f) - double(b_f),
 *   p = diff * diff, acc = acc + p, three separately rounded operations (no fma).  Always differences per feature.
 * vgan_inne_build: the T estimators of the subspaces first .. first + count - 1 of the table (feat, feat_off: the feature
 *   lists, concatenated, and their offsets) from X [n, d] (ldx), 2 <= psi <= n <= 2^31 - 1, into their slots of the four
 *   arrays.  Estimator (s, t) has the stream id = s T + t: centre j is row feistel_perm(j, n, seed, id), j < psi (the
 *   permutation of vgan_shuffle_index), in that order.  nn_j is the position i != j with the smallest (d2(c_j, c_i), i),
 *   r2_j = d2(c_j, c_nn_j); comparisons on d2, never on square roots.  With eps = 2^-52, ratio VGAN_INNE_RATIO_SQUARED:
 *   rho_j = 1.0 - (r2[nn_j] + eps) / (r2_j + eps); VGAN_INNE_RATIO_DISTANCE: the same on sqrt(r2); float64, every
 *   operation rounded on its own.  One workgroup per estimator, the row indices in LDS, the psi x psi matrix is never
 *   stored; no workspace.  max_dims: no subspace of the range has more features (at most VGAN_INNE_MAX_DIMS).  The same
 *   bits from run to run and for every split of the subspaces over calls.  count <= 65535.
 * vgan_inne_scores: score float32 [count, ld_score] (ld_score >= nq): for every query row x of Xq [nq, d] (ldq) and every
 *   subspace of the range float32(sum_t iso_t / double(T)), the sum in float64 with t ascending; iso_t = rho_j of the centre
 *   j of estimator t with the smallest (r2_j, j) among those with d2(x, c_j) <= r2_j, 1.0 where there is none.  X [n, d]
 *   (ldx) is the matrix the estimators were built from (the centres are read from it by row index).  No atomics, no
 *   workspace: the same bits for every split of the rows or the subspaces over calls.  count <= 65535.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_INNE_MAX_SAMPLES 1024
#define VGAN_INNE_MAX_ESTIMATORS 1024
#define VGAN_INNE_MAX_DIMS 8192
#define VGAN_INNE_RATIO_SQUARED 0
#define VGAN_INNE_RATIO_DISTANCE 1
int vgan_inne_build(const float* X, int ldx, int64_t n, int d, const int32_t* feat, const int32_t* feat_off, int first,
                    int count, int max_dims, int T, int psi, int ratio, uint64_t seed, int32_t* rows, double* r2, int32_t* nn,
                    double* rho, vgan_stream_t stream);
int vgan_inne_scores(const float* Xq, int ldq, int nq, int d, const float* X, int ldx, int64_t n, const int32_t* feat,
                     const int32_t* feat_off, int first, int count, int max_dims, int T, int psi, const int32_t* rows,
                     const double* r2, const double* rho, float* score, int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mahalanobis / MCD outlier scores (sklearn's EmpiricalCovariance / ShrunkCovariance / OAS .mahalanobis; pyod's MCD up to the
 * estimator): a float64 mean and covariance per subspace, the shrunk matrix's Cholesky factor inverted, and the squared
 * distance as a triangular product  (v-gan_amd/outlier.py: SubspaceMahalanobis, whose docstring is the definition; kernels
 * in csrc/outlier_maha.hip).  X is float32, all arithmetic float64.  Subspaces are positions of a SUBSPACE TABLE (feat,
 * feat_off); sq_off int64 [S + 1] is the running sum of d_s^2: the d_s x d_s row-major matrices of subspace s (cov, L, W)
 * start at element sq_off[s], its mean at element feat_off[s].  Every entry works on the range first .. first + count - 1
 * (count <= 65535), max_dims >= every d_s of the range, d_s <= VGAN_MAHA_MAX_DIMS.  hcount int32 [S]: h_s, the rows of the
 * support.  support uint8 [S, ld_support], 1 = the row is in H_s; NULL: every row (then h_s = n).
 * vgan_maha_moments: mean = (1 / h_s) sum_{i in H_s} x_i and cov = C_s = (1 / h_s) sum_{i in H_s} (x_i - mu)(x_i - mu)^T (biased,
 *   two passes, both triangles written) from X [n, d] (ldx), 2 <= n <= VGAN_MAHA_MAX_ROWS.  The rows are cut into slabs of
 *   VGAN_MAHA_SLAB_ROWS rows by n alone; a slab's sum has a fixed order (the covariance on the f64 matrix unit, 16 x 16
 *   tiles of the lower triangle) and the slabs are added in ascending order, so the bits do not depend on the workspace,
 *   which only sets how many slabs and tiles one launch takes.  tiles int32 [n_tiles, 3]: (s, ti, tj), tj <= ti <
 *   ceil(d_s / 16), every lower-triangle tile of every subspace of the range; total_dims = the sum of d_s over the range.
 *   workspace: at least 8 * total_dims and at least 2048 bytes.
 * vgan_maha_factor: per subspace m = tr C / d, alpha = shrinkage, or for VGAN_MAHA_SHRINKAGE_OAS: a = mean(C_ij^2), alpha = 1
 *   if (h + 1)(a - m^2 / d) == 0 else min((a + m^2) / ((h + 1)(a - m^2 / d)), 1) (sklearn's oas); cov is overwritten with
 *   Sigma = (1 - alpha) C + alpha m I; L receives its lower Cholesky factor (blocked right-looking, the trailing update on
 *   the f64 matrix unit), W = L^-1 (lower triangular, zeros above).  status int32 [S] (zeroed by the caller before the
 *   first call of a fit): bit 0 = tr C == 0 in this call (W = 0: every score is exactly 0), bit 1 = a pivot was not
 *   positive and finite in this or an earlier call (L, W unspecified).  One workgroup per subspace.
 * vgan_maha_scores: score[s, i] = float32(|| W_s (x_i - mu_s) ||^2) for the rows of Xq [rows, d] (ldq) into score [S,
 *   ld_score], row s; the product on the f64 matrix unit, K in ascending order up to the diagonal, then the squares in
 *   ascending order: the bits of an element do not depend on where its row sits in the call.
 * vgan_maha_select: support[s, i] = 1 for the h_s rows with the smallest (score[s, i], i), -0.0 taken as +0.0, else 0;
 *   changed[s] = 1 if that differs from what support held before, else 0.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_MAHA_MAX_DIMS 1024
#define VGAN_MAHA_MAX_ROWS 16777216 /* 2^24 */
#define VGAN_MAHA_SLAB_ROWS 1024
#define VGAN_MAHA_SHRINKAGE_OAS (-1.0)
#define VGAN_MAHA_STATUS_CONSTANT 1
#define VGAN_MAHA_STATUS_PIVOT 2
int vgan_maha_moments(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off,
                      const int64_t* sq_off, int first, int count, int total_dims, int max_dims, const int32_t* tiles,
                      int n_tiles, const uint8_t* support, int64_t ld_support, const int32_t* hcount, double* mean,
                      double* cov, void* workspace, int64_t workspace_bytes, vgan_stream_t stream);
int vgan_maha_factor(double* cov, const int64_t* sq_off, const int32_t* feat_off, int first, int count, int max_dims,
                     const int32_t* hcount, double shrinkage, double* L, double* W, double* alpha, int32_t* status,
                     vgan_stream_t stream);
int vgan_maha_scores(const float* Xq, int ldq, int rows, int d, const int32_t* feat, const int32_t* feat_off,
                     const int64_t* sq_off, int first, int count, int max_dims, const double* mean, const double* W,
                     float* score, int64_t ld_score, vgan_stream_t stream);
int vgan_maha_select(const float* score, int64_t ld_score, int n, int first, int count, const int32_t* hcount,
                     uint8_t* support, int64_t ld_support, int32_t* changed, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian-mixture outlier scores (sklearn's GaussianMixture with covariance_type "full", n_init 1; pyod's GMM): EM for
 * n_components = C full-covariance Gaussians per subspace and score = -log sum_c w_c N(x; mu_c, Sigma_c)  (v-gan_amd/outlier.py:
 * SubspaceGMM, whose docstring is the definition; kernels in csrc/outlier_gmm.hip).  X is float32, all arithmetic float64.
 * The (subspace, component) pairs are the entries e = s C + c of an EXPANDED subspace table: feat holds the feature list of
 * every subspace C times, feat_off int32 [S C + 1] and sq_off int64 [S C + 1] (running sum of d_s^2) accordingly; mean at
 * feat_off[e], cov / L / W at sq_off[e], nk, weights, log_weights, logdet and the factor's status at e.  With that table
 * vgan_maha_factor(shrinkage = 0) on the entries first C .. (first + count) C - 1 gives L and W of every component and leaves
 * cov as it is.  Every entry below works on the SUBSPACES first .. first + count - 1, count C <= 65535, 1 <= C <=
 * VGAN_GMM_MAX_COMPONENTS, max_dims >= every d_s of the range, d_s <= VGAN_MAHA_MAX_DIMS.  resp float64 [count, C, n]: the
 * responsibilities of the range.  done int32 [S] (NULL: none): a subspace whose flag is not 0 is frozen, its workgroups
 * return at once and nothing of it is written.
 * vgan_gmm_moments: nk_c = sum_i r_ic + 10 eps, mu_c = sum_i r_ic x_i / nk_c, cov = Sigma_c = sum_i r_ic (x_i - mu_c)(x_i -
 *   mu_c)^T / nk_c + reg_covar I (two passes, both triangles written), weights = nk_c / sum_c nk_c (c ascending), log_weights
 *   its logarithm; from X [n, d] (ldx), 2 <= n <= VGAN_MAHA_MAX_ROWS.  The rows are cut into slabs of VGAN_MAHA_SLAB_ROWS
 *   rows by n alone; a slab's sum has a fixed order (the covariance on the f64 matrix unit with A = r (x - mu), B = x - mu)
 *   and the slabs are added in ascending order, so the bits do not depend on the workspace.  tiles int32 [n_tiles, 3]: (e,
 *   ti, tj), tj <= ti < ceil(d_e / 16), every lower-triangle tile of every entry of the range; total_dims = the sum of d_e
 *   over the entries of the range.  workspace: at least 8 (total_dims + count C) and at least 2048 bytes.
 * vgan_gmm_logdet: logdet[e] = sum_j log L_e[j, j], a fixed order.
 * vgan_gmm_estep: lp_ic = -0.5 (d_s log 2pi + ||W_c (x_i - mu_c)||^2) - logdet_c + log w_c for the rows of Xq [rows, d] (ldq),
 *   the product as in vgan_maha_scores with the float64 square sum kept; ln_i = logsumexp_c lp_ic (the maximum subtracted,
 *   c ascending).  resp (or NULL) receives exp(lp_ic - ln_i), evaluated as exp(lp_ic - max) / sum_c exp(lp_ic - max) so that a row
 *   sums to 1 within a few ulps whatever the size of ln_i; score (or NULL; float32 [S, ld_score], row s) receives
 *   float32(-ln_i); lb_partial (or NULL; float64 [count, ceil(rows / 64)], needs resp) the sum of ln_i over each 64 rows in a
 *   fixed order.  At least one of resp and score is given.  The bits of a row do not depend on where it sits in the call.
 *   d and max_dims are only range-checked here (ldq >= d > 0, 1 <= max_dims <= VGAN_MAHA_MAX_DIMS): the kernel's LDS need does
 *   not depend on d_s, so max_dims sizes nothing, and the entries of feat are the caller's to keep below d, as for
 *   vgan_maha_scores.  Both stay in the signature so that the entry reads like the other subspace-table entries.
 * vgan_gmm_converge: per subspace that is not done: if any status[e] of it is not 0: done = VGAN_GMM_DONE_FAILED.  Otherwise,
 *   for iteration >= 1: lb = (sum of lb_partial, each slab of VGAN_MAHA_SLAB_ROWS rows in order, the slabs ascending) / n,
 *   n_iter = iteration, lower_bound = lb; |lb - lb_prev| < tol sets done = VGAN_GMM_DONE_CONVERGED, otherwise lb_prev = lb
 *   (the caller starts lb_prev at -inf).  iteration 0 only looks at the status (lb_partial may be NULL).  lb_partial is
 *   overwritten.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_GMM_MAX_COMPONENTS 32
#define VGAN_GMM_DONE_CONVERGED 1
#define VGAN_GMM_DONE_FAILED 2
int vgan_gmm_moments(const float* X, int ldx, int n, int d, const int32_t* feat, const int32_t* feat_off,
                     const int64_t* sq_off, int n_components, int first, int count, int total_dims, int max_dims,
                     const int32_t* tiles, int n_tiles, const double* resp, const int32_t* done, double reg_covar, double* nk,
                     double* weights, double* log_weights, double* mean, double* cov, void* workspace,
                     int64_t workspace_bytes, vgan_stream_t stream);
int vgan_gmm_logdet(const double* L, const int32_t* feat_off, const int64_t* sq_off, int n_components, int first, int count,
                    double* logdet, vgan_stream_t stream);
int vgan_gmm_estep(const float* Xq, int ldq, int rows, int d, const int32_t* feat, const int32_t* feat_off,
                   const int64_t* sq_off, int n_components, int first, int count, int max_dims, const double* mean,
                   const double* W, const double* logdet, const double* log_weights, const int32_t* done, double* resp,
                   double* lb_partial, float* score, int64_t ld_score, vgan_stream_t stream);
int vgan_gmm_converge(double* lb_partial, int n, int n_components, int first, int count, const int32_t* status, double tol,
                      int iteration, int32_t* done, int32_t* n_iter, double* lower_bound, double* lb_prev,
                      vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PCA outlier scores (pyod's PCA as its documentation describes it; sklearn's StandardScaler + PCA for the spectrum): the
 * eigenpairs of the covariance or correlation matrix of every subspace and score = sum_j w_j y_j^2, y = V D^-1 (x - mu)
 * (v-gan_amd/outlier.py: SubspacePCA, whose docstring is the definition; kernels in csrc/outlier_pca.hip).  mean and cov come
 * from vgan_maha_moments; the SUBSPACE TABLE (feat, feat_off, sq_off), first, count (<= 65535) and max_dims (>= every d_s of
 * the range, d_s <= VGAN_MAHA_MAX_DIMS) are as for the vgan_maha_* entries.  All arithmetic is float64.
 * vgan_pca_eigen: per subspace scale_k = sqrt(C_kk), a scale of exactly 0 replaced by 1, and M_ij = C_ij / (scale_i scale_j)
 *   when standardize is 1; scale_k = 1 and M = C when it is 0.  M = V^T diag(evals) V by a cyclic two-sided Jacobi method
 *   with a fixed parallel order: a sweep is n - 1 rounds of a round-robin tournament on n = d_s rounded up to even players
 *   (round r: position 0 holds player n - 1, position k >= 1 player (k - 1 + r) mod (n - 1); pair i = the players (a, b) at
 *   positions i and n - 1 - i; a pair with a player >= d_s rests).  A pair is skipped when |m_ab| <= 2^-53 sqrt(|m_aa m_bb|);
 *   otherwise zeta = (m_bb - m_aa) / (2 m_ab), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t, every
 *   pair of the round from the matrix as the previous round left it.  The rotations of a round act on disjoint index pairs;
 *   M <- J^T M J is evaluated per 2 x 2 block (pair I, pair J), I <= J, as R_I^T (B R_J) with R = [c s; -s c], the mirror image
 *   written with it, the block I = I set to diag(m_aa - t m_ab, m_bb + t m_ab); the rows a, b of V turn as c v_a - s v_b, s v_a
 *   + c v_b.  A sweep in which no pair rotated ends the subspace; at most max_sweeps (>= 1) sweeps run.  sweeps int32 [S]: the
 *   sweeps run, the last, rotation-free one included.  status int32 [S] (written, not accumulated): bit 0 = tr M == 0, bit
 *   1 = max_sweeps sweeps ran and the last one still rotated.  evals (float64 at feat_off[s]) = the diagonal of the final M
 *   in descending order, ties by the ascending diagonal position; V (float64 [d_s, d_s] at sq_off[s]): row j the unit
 *   eigenvector of evals[j], signed so that its entry of largest magnitude (the lowest index on a tie) is positive.  scale
 *   float64 at feat_off[s].  cov is overwritten and unspecified afterwards.  One workgroup per subspace; M and V live in
 *   LDS for d_s <= VGAN_PCA_LDS_DIMS and in cov / V beyond.  The order is fixed, so the bits are.
 * vgan_pca_scores: score[s, i] = float32(sum_j wt_j y_ij^2), y_ij = sum_k V_s[j, k] ((x_ik - mu_k) inv_scale_k), for the rows of
 *   Xq [rows, d] (ldq) into score [S, ld_score], row s.  inv_scale and wt are float64 at feat_off[s]; wt_j is the weight of
 *   component j, 0 for a component outside the wanted set.  The product runs on the f64 matrix unit, K in ascending order
 *   over all d_s; a 16-row tile of V whose weights are all 0 is skipped, which depends on wt alone.  The squares are added
 *   per residue j mod 4 in ascending j, then the four as (r0 + r1) + (r2 + r3): the bits of an element do not depend on where
 *   its row sits in the call.
 * Both return VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_PCA_LDS_DIMS 48
#define VGAN_PCA_STATUS_CONSTANT 1
#define VGAN_PCA_STATUS_NOT_CONVERGED 2
int vgan_pca_eigen(double* cov, const int64_t* sq_off, const int32_t* feat_off, int first, int count, int max_dims,
                   int standardize, int max_sweeps, double* scale, double* evals, double* V, int32_t* sweeps, int32_t* status,
                   vgan_stream_t stream);
int vgan_pca_scores(const float* Xq, int ldq, int rows, int d, const int32_t* feat, const int32_t* feat_off,
                    const int64_t* sq_off, int first, int count, int max_dims, const double* mean, const double* inv_scale,
                    const double* V, const double* wt, float* score, int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One-class SVM outlier scores (Schoelkopf et al. 2001; sklearn's OneClassSVM with the RBF kernel, shrinking off; pyod's
 * OCSVM): K_s(x, y) = exp(-gamma_s d_s(x, y)^2), the dual min 1/2 a^T K a, 0 <= a_t <= 1, sum a = nu n by SMO, score = rho -
 * sum_r a_r K_s(x_r, x) (v-gan_amd/outlier.py: SubspaceOCSVM, whose docstring is the definition; kernels in
 * csrc/outlier_ocsvm.hip).  The packed blocks, squared norms, SUBSPACE TABLE (feat_off, col_off), first, count (<= 65535),
 * engine and splits are those of vgan_outlier_kde; gamma float64 [S], indexed by first + z.  2 <= n <= VGAN_OCSVM_MAX_ROWS.
 * vgan_ocsvm_kernel_matrix: K float32 [count, n, n]; K[z][c][q] = float32 exp of float32(-gamma_s d2(q, c)), d2 the engine's
 *   float32 squared distance of query row q and reference row c of the one block P; the diagonal is exactly 1.  Every entry
 *   is written once whatever splits is.
 * vgan_ocsvm_init: libsvm's start for the chunk's count matrices: alpha[z][t] = 1 for t < m, a_m for t = m (m < n needs 0 <=
 *   a_m < 1, m = n needs a_m = 0; m = 0 needs a_m > 0), 0 beyond; G[z][t] = sum over the rows r with alpha_r != 0, ascending,
 *   of (double)K[z][r][t] alpha_r, every product and sum rounded; done[z] = n_iter[z] = 0.  alpha, G float64 [count, n].
 * vgan_ocsvm_smo: at most `iterations` steps of WSS2 (Fan, Chen, Lin 2005) for every chunk subspace whose done[z] is 0, one
 *   workgroup each, float64 with K widened, every operation rounded on its own (no FMA).  A step: stop with done =
 *   VGAN_OCSVM_DONE_MAX_ITER if n_iter >= max_iter; i = the lowest index with the largest -G_t among alpha_t < 1, Gmax = -G_i,
 *   Gmax2 = the largest G_t among alpha_t > 0; stop with done = VGAN_OCSVM_DONE_CONVERGED if there is no i or Gmax + Gmax2 <
 *   tol; among alpha_t > 0 with b_t = Gmax + G_t > 0 and q_t = 2.0 - 2.0 K[i][t] (1e-12 if <= 0), j = the lowest index with the
 *   smallest -(b_t b_t) / q_t, stop as converged if there is none; delta = (G_i - G_j) / q_j, s = alpha_i + alpha_j, alpha_i -=
 *   delta, alpha_j += delta, libsvm's four clips for equal labels with C = 1; G_t = G_t + (K[i][t] da_i + K[j][t] da_j) for every
 *   t; n_iter += 1.  A subspace that reaches max_iter updates inside a launch is flagged in that launch.  A stopped
 *   subspace is not touched again.  storage: where alpha and G live during a launch and how wide the workgroup is:
 *   VGAN_OCSVM_STORAGE_LDS (in LDS, 256 threads, n <= VGAN_OCSVM_LDS_ROWS), _GLOBAL (in place, 256 threads), _WIDE (in place,
 *   1024 threads) or _AUTO (LDS when it fits, WIDE beyond); the results are the same bits.  tol > 0, max_iter >= 1,
 *   iterations >= 1: no launch loops unbounded.
 * vgan_ocsvm_rho: rho[z] = the mean of G_t over 0 < alpha_t < 1 (a fixed order); with no such row (max G over alpha_t = 1 + min
 *   G over alpha_t = 0) / 2, and with one of the two sets empty as well the other one's bound.
 * vgan_ocsvm_scores: score[score_row[z] (or z), q] = float32((rint(rho_s 2^44) - sum_r rint(alpha_r K_s(x_r, q) 2^44)) 2^-44) for
 *   the nq rows of Pq against the nr fitted rows of Pr, K_s as in vgan_ocsvm_kernel_matrix without the diagonal rule, rows
 *   with alpha_r = 0 skipped; alpha float64 [S, nr] and rho float64 [S] indexed by first + z.  acc uint64 [count nq] is
 *   scratch.  The integer sum has no order: the bits do not depend on splits or on the chunk.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_OCSVM_MAX_ROWS 32768
#define VGAN_OCSVM_LDS_ROWS 2048
#define VGAN_OCSVM_DONE_CONVERGED 1
#define VGAN_OCSVM_DONE_MAX_ITER 2
#define VGAN_OCSVM_STORAGE_AUTO 0
#define VGAN_OCSVM_STORAGE_GLOBAL 1
#define VGAN_OCSVM_STORAGE_LDS 2
#define VGAN_OCSVM_STORAGE_WIDE 3
int vgan_ocsvm_kernel_matrix(const float* P, const float* sq, int n, const int32_t* feat_off, const int64_t* col_off, int first,
                             int count, const double* gamma, int engine, int splits, float* K, vgan_stream_t stream);
int vgan_ocsvm_init(const float* K, int n, int count, int m, double a_m, double* alpha, double* G, int32_t* done,
                    int32_t* n_iter, vgan_stream_t stream);
int vgan_ocsvm_smo(const float* K, int n, int count, double tol, int max_iter, int iterations, int storage, double* alpha,
                   double* G, int32_t* done, int32_t* n_iter, vgan_stream_t stream);
int vgan_ocsvm_rho(const double* alpha, const double* G, int n, int count, double* rho, vgan_stream_t stream);
int vgan_ocsvm_scores(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                      const int32_t* feat_off, const int64_t* col_off, int first, int count, const double* gamma,
                      const double* alpha, const double* rho, int engine, int splits, uint64_t* acc, float* score,
                      const int32_t* score_row, int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Stochastic outlier selection (Janssens, Huszar, Postma, van den Herik 2012; pyod's SOS; the perplexity search of t-SNE):
 * every fitted row i gets a width beta_i at which the entropy of its affinities exp(-beta_i (D[i, j] - dmin_i)) over the other
 * rows equals log(perplexity); a row's score is the probability that no fitted row binds to it (v-gan_amd/outlier.py:
 * SubspaceSOS, whose docstring is the definition; kernels in csrc/outlier_sos.hip).  The packed blocks, squared norms, SUBSPACE
 * TABLE (feat_off, col_off), first, count (<= 65535), engine and splits are those of vgan_outlier_kde.  VGAN_SOS_MIN_ROWS <= n
 * <= VGAN_SOS_MAX_ROWS.  metric: VGAN_SOS_METRIC_EUCLIDEAN (a dissimilarity is sqrtf of the engine's float32 d2) or
 * _SQEUCLIDEAN (d2 itself).
 * vgan_sos_distance_matrix: D float32 [count, n, n]; D[z][c][q] = the dissimilarity of query row q and reference row c of the one
 *   block P.  Every entry is written once whatever splits is; the diagonal is written and never read by the entries below.
 * vgan_sos_fit: for every row i of the chunk's count matrices, all float64 with D widened, every operation rounded on its own (no
 *   FMA): dmin = min_j D[i][j] and m = the number of j with D[i][j] = dmin, over j != i.  m >= perplexity: beta = inf, Z = m,
 *   n_iter = 0, flags = VGAN_SOS_FLAG_DEGENERATE.  Otherwise beta = 1, lo = 0, hi = inf and, at every step, a_j = exp(-(beta e_j)),
 *   e_j = D[i][j] - dmin, Z = sum a_j, diff = (log(Z) + beta ((sum e_j a_j) / Z)) - log(perplexity), the logarithm of perplexity
 *   taken once on the host; stop if |diff| <= tol; stop with flags = VGAN_SOS_FLAG_UNCONVERGED if max_iter updates have run;
 *   diff > 0: lo = beta, beta = 2 beta while hi is inf, else (beta + hi) / 2; diff <= 0: hi = beta, beta = (beta + lo) / 2; n_iter
 *   counts the updates.  beta, dmin, Z float64 [count, n] (Z at the final beta), n_iter, flags int32 [count, n].  The order of the
 *   two sums is the kernel's own.  storage: VGAN_SOS_STORAGE_WAVE (a row's entries in the registers of one wave, four rows per
 *   workgroup, n <= VGAN_SOS_WAVE_ROWS), _BLOCK (in those of a workgroup of 1024 threads) or _AUTO (WAVE where it fits).
 *   1 < perplexity < n - 1, tol > 0 and finite, max_iter >= 1: no launch loops unbounded.
 * vgan_sos_fit_scores: score[score_row[z] (or z), j] = float32(exp(-(sum_{i != j} rint(min(-log1p(-min(a_i / Z_i, 1)), 128) 2^40))
 *   2^-40)) with a_i = exp(-(beta_i (D[z][j][i] - dmin_i))), or for beta_i = inf 1 if D[z][j][i] <= dmin_i, else 0: the fitted
 *   rows scored from the chunk's stored matrices; beta, dmin, Z float64 [count, n].
 * vgan_sos_scores: the same for the nq new rows of Pq against the nr fitted rows of Pr, the dissimilarity from the engine with
 *   the new row as query, no row left out and the term min(log1p(a_i / Z_i), 128): the new row appended to the fitted set.  beta,
 *   dmin, Z float64 [S, nr] indexed by first + z.  acc uint64 [count nq] is scratch.
 * The integer sums have no order: the bits of a score do not depend on splits or on the chunk.  Every entry returns
 * VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_SOS_MIN_ROWS 3
#define VGAN_SOS_MAX_ROWS 32768
#define VGAN_SOS_WAVE_ROWS 2048
#define VGAN_SOS_METRIC_EUCLIDEAN 0
#define VGAN_SOS_METRIC_SQEUCLIDEAN 1
#define VGAN_SOS_STORAGE_AUTO 0
#define VGAN_SOS_STORAGE_WAVE 1
#define VGAN_SOS_STORAGE_BLOCK 2
#define VGAN_SOS_FLAG_DEGENERATE 1
#define VGAN_SOS_FLAG_UNCONVERGED 2
int vgan_sos_distance_matrix(const float* P, const float* sq, int n, const int32_t* feat_off, const int64_t* col_off, int first,
                             int count, int metric, int engine, int splits, float* D, vgan_stream_t stream);
int vgan_sos_fit(const float* D, int n, int count, double perplexity, double tol, int max_iter, int storage, double* beta,
                 double* dmin, double* Z, int32_t* n_iter, int32_t* flags, vgan_stream_t stream);
int vgan_sos_fit_scores(const float* D, int n, int count, const double* beta, const double* dmin, const double* Z, float* score,
                        const int32_t* score_row, int64_t ld_score, vgan_stream_t stream);
int vgan_sos_scores(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                    const int32_t* feat_off, const int64_t* col_off, int first, int count, int metric, const double* beta,
                    const double* dmin, const double* Z, int engine, int splits, uint64_t* acc, float* score,
                    const int32_t* score_row, int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Local correlation integral over a fixed grid of radii (LOCI: Papadimitriou, Kitagawa, Gibbons, Faloutsos 2003; pyod's LOCI):
 * a row's neighbour count within alpha r is compared with the counts of the rows within r of it, at every radius r of the grid,
 * and the score is the largest deviation in units of the local standard deviation (v-gan_amd/outlier.py: SubspaceLOCI, whose
 * docstring is the definition; kernels in csrc/outlier_loci.hip).  D float32 [count, n, n] is the Euclidean matrix,
 * D[z][c][q] with the subject row q contiguous; every entry below takes its diagonal as 0 whatever is
 * stored.  VGAN_LOCI_MIN_ROWS <= n <= VGAN_LOCI_MAX_ROWS, 1 <= R <= VGAN_LOCI_MAX_RADII, count <= 65535.  r (sampling radii)
 * and a (counting radii, alpha r) are float32 [count, R], ascending, formed by the caller; all comparisons are float32.
 * vgan_loci_distance_matrix: D as vgan_sos_distance_matrix writes it with VGAN_SOS_METRIC_EUCLIDEAN (the same arguments, layout
 *   and bits: sqrtf of the engine's float32 d2 with row q as the query), from VGAN_LOCI_MIN_ROWS = 2 rows on.
 * vgan_loci_rmax: rmax float32 [count], the largest off-diagonal entry of every matrix (0 where all are 0): an exact maximum
 *   without an order, from which the caller forms r and a.
 * vgan_loci_counts: cnt int32 [count, n, R], cnt[z][q][j] = #{c : D[z][c][q] <= a[z][j]} (the row itself included).
 * vgan_loci_sums: over the rows c with D[z][c][p] <= r[z][j]: m int32 their number, S1 int64 the sum of cnt[z][c][j], S2 int64
 *   the sum of cnt[z][c][j]^2; all [count, n, R].
 * vgan_loci_finish: num = S1 - cnt m and den = m S2 - S1^2 in int64 (exact: both products stay below 2^60); radius j is valid
 *   iff m >= n_min and den > 0; score[score_row[z] (or z), p] = float32(max(0, max over the valid j of float64(num) /
 *   sqrt(float64(den)))); best (int32, the layout of score, may be null) the lowest j that attains a positive maximum, else -1.
 * vgan_loci_scores: the nq new rows of Pq against the nr fitted rows of Pr (the packed blocks, squared norms, SUBSPACE TABLE,
 *   first, count, engine and splits of vgan_sos_scores), each scored alone as appended to the fitted set: with d = sqrtf of the
 *   engine's d2 (the new row as query), A = #{d <= a_j}, M = #{d <= r_j}, T1 / T2 = the sums of cnt[c][j] / cnt[c][j]^2 over the
 *   rows counted in M, added as 64-bit integers into acc uint64 [count, nq, 4, R] (scratch, zeroed by the entry); then cnt = A +
 *   1, m = M + 1, S1 = T1 + cnt, S2 = T2 + cnt^2 and the rule of vgan_loci_finish.  r, a float32 [S, R] and cnt int32 [S, nr, R]
 *   are indexed by first + z.  dist_out (may be null; count must be 1): float32 [nq, nr], the distances that were counted.
 * The integer sums have no order: no result depends on splits or on the chunk.  Every entry returns VGAN_ERR_ARG before
 * touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_LOCI_MIN_ROWS 2
#define VGAN_LOCI_MAX_ROWS 32768
#define VGAN_LOCI_MAX_RADII 64
int vgan_loci_distance_matrix(const float* P, const float* sq, int n, const int32_t* feat_off, const int64_t* col_off, int first,
                              int count, int engine, int splits, float* D, vgan_stream_t stream);
int vgan_loci_rmax(const float* D, int n, int count, float* rmax, vgan_stream_t stream);
int vgan_loci_counts(const float* D, int n, int count, const float* a, int R, int32_t* cnt, vgan_stream_t stream);
int vgan_loci_sums(const float* D, int n, int count, const float* r, int R, const int32_t* cnt, int32_t* m, int64_t* S1, int64_t* S2,
                   vgan_stream_t stream);
int vgan_loci_finish(const int32_t* cnt, const int32_t* m, const int64_t* S1, const int64_t* S2, int n, int count, int R, int n_min,
                     float* score, const int32_t* score_row, int64_t ld_score, int32_t* best, vgan_stream_t stream);
int vgan_loci_scores(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int nr,
                     const int32_t* feat_off, const int64_t* col_off, int first, int count, const float* r, const float* a,
                     const int32_t* cnt, int R, int n_min, int engine, int splits, uint64_t* acc, float* dist_out, float* score,
                     const int32_t* score_row, int64_t ld_score, int32_t* best, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Subspace outlier degree (SOD: Kriegel, Kroeger, Schubert, Zimek 2009; pyod's SOD): a row is judged against the rows that
 * share the most nearest neighbours with it, in the features in which those rows vary little (v-gan_amd/outlier.py:
 * SubspaceSOD, whose docstring is the definition; kernels in csrc/outlier_sod.hip).  Lists are the refined lists of
 * vgan_outlier_refine, int32 [count, rows, k], 1 <= k <= VGAN_OUTLIER_MAX_K; count <= 65535.
 * vgan_sod_reverse_lists: the reverse lists of the fit-time lists idx [count, n, k] as a CSR per subspace: RN(m) = the rows
 *   whose list holds m = rn_rows[z, rn_off[z, m] .. rn_off[z, m + 1]) (rn_off int32 [count, n + 1], rn_rows int32 [count, n k]),
 *   by an integer count, an exclusive scan and a fill.  The order of the rows inside one RN(m) is not specified: only integer
 *   counts are formed from it.  cursor int32 [count, n] is scratch.  k < n <= VGAN_SOD_MAX_ROWS.  An entry outside [0, n) is
 *   skipped (the lists of vgan_outlier_refine hold none).
 * vgan_sod_reference_sets: refset[z, q, 0 .. ref_set) (int32 [count, nq, ref_set]) = the first ref_set fitted rows j in the
 *   order (SNN(q, j) descending, j ascending), SNN(q, j) = |N(q) n N(j)| with N(q) = idxq[z, q, .] and N(j) the fit-time list
 *   behind the CSR; rows with SNN = 0 take part.  exclude_self != 0 (fit: nq == nr, query q is fitted row q): j = q is left
 *   out.  n_unshared (int32 [count], may be NULL): the number of query rows whose set took a row with SNN = 0.  The counts
 *   are integers held as packed bytes in LDS, a table of one byte per fitted row, which is what bounds nr <=
 *   VGAN_SOD_MAX_ROWS; the sets do not depend on the launch.  1 <= ref_set <= VGAN_SOD_MAX_REF, ref_set <= nr (nr - 1 with
 *   exclude_self), k < nr.
 * vgan_sod_score: per chunk subspace s = first + z (features F_s ascending, d_s of them; SUBSPACE TABLE feat / feat_off) and
 *   query row q with R = refset[z, q, .]: mu_f = (sum_{r in R, in order} Xr[r, f]) / ref_set, v_f = (sum_{r in R, in order}
 *   (Xr[r, f] - mu_f)^2) / ref_set, float64 from the raw float32 values, every operation rounded on its own (no FMA).  V =
 *   sum_f v_f in this shape: 64 partial sums, partial l over the positions l, l + 64, ... of F_s ascending, then the partials
 *   in order l = 0 .. 63.  T = (alpha V) / d_s; f is relevant iff v_f < T; r = the number of relevant features; Q = the sum
 *   of (Xq[q, f] - mu_f)^2 over the relevant f in the same shape.  score = sqrt(Q / r) (VGAN_SOD_FORM_PYOD) or sqrt(Q) / r
 *   (VGAN_SOD_FORM_PAPER), 0 where r = 0, rounded once to float32 (row and ld_score as for vgan_outlier_score).
 *   n_relevant[z, q] = r (int32 [count, nq]).  mask (uint32 [count, nq, mask_words], may be NULL): bit i % 32 of word i / 32
 *   is set iff position i of F_s is relevant; words at or past mask_words are not written, words past ceil(d_s / 64) 2 are
 *   left as they are.  An entry of refset outside [0, nr) counts as a row at the origin.  0 < alpha <= 1.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_SOD_MAX_ROWS 32768
#define VGAN_SOD_MAX_REF 64
#define VGAN_SOD_FORM_PYOD 0
#define VGAN_SOD_FORM_PAPER 1
int vgan_sod_reverse_lists(const int32_t* idx, int n, int k, int count, int32_t* rn_off, int32_t* rn_rows, int32_t* cursor,
                           vgan_stream_t stream);
int vgan_sod_reference_sets(const int32_t* idxq, int nq, const int32_t* rn_off, const int32_t* rn_rows, int nr, int k, int count,
                            int ref_set, int exclude_self, int32_t* refset, int32_t* n_unshared, vgan_stream_t stream);
int vgan_sod_score(const float* Xq, int ldq, int nq, const float* Xr, int ldr, int nr, int d, const int32_t* feat,
                   const int32_t* feat_off, int first, int count, const int32_t* refset, int ref_set, double alpha, int form,
                   float* score, const int32_t* score_row, int ld_score, int32_t* n_relevant, uint32_t* mask, int mask_words,
                   vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel PCA novelty scores (Hoffmann 2007: the reconstruction error in feature space; sklearn's KernelPCA for the
 * decomposition; pyod's KPCA): K_s(x, y) = exp(-gamma_s d_s(x, y)^2) over m landmark rows, the eigenpairs of the centred
 * kernel matrix, score = max(pot - sum_j w_j y_j^2, 0) (v-gan_amd/outlier.py: SubspaceKPCA, whose docstring is the
 * definition; kernels in csrc/outlier_kpca.hip).  The kernel matrix is vgan_ocsvm_kernel_matrix's on the packed landmark
 * block and the eigenpairs are vgan_pca_eigen's (standardize 0) with the synthetic tables feat_off = [0, m, 2 m, ...] and
 * sq_off = [0, m^2, 2 m^2, ...].  The packed blocks, squared norms, SUBSPACE TABLE (feat_off, col_off), first, count (<=
 * 65535), engine and splits are those of vgan_outlier_kde; gamma float64 [S], indexed by first + z.  2 <= m <=
 * VGAN_KPCA_MAX_LANDMARKS (the eigensolver's VGAN_MAHA_MAX_DIMS).
 * vgan_kpca_center: K float32 [count, m, m].  Only the entries K[z][r][c] with r <= c are read; K' is the symmetric matrix
 *   they define.  col_mean[z][c] (float64 [count, m]) = (the sum of K'[r][c] over r ascending) / m; total[z] (float64 [count]) =
 *   (the sum of col_mean[z][c] over c ascending) / m; Kc[z][i][j] (float64 [count, m, m], the layout vgan_pca_eigen reads with
 *   the synthetic sq_off) = ((K'[i][j] - col_mean_j) - col_mean_i) + total for i <= j, written to both places: Kc is symmetric
 *   to the bit.  Every operation is rounded on its own; there is no product.
 * vgan_kpca_kernel_rows: R float32 [count, nq, m]; R[z][q][c] = float32 exp of float32(-gamma_s d2(q, c)), d2 the engine's
 *   float32 squared distance of query row q of Pq and landmark row c of Pr (vgan_ocsvm_kernel_matrix's entry without the
 *   diagonal rule).  Every entry is written once whatever splits is.  0 < nq <= VGAN_MAHA_MAX_ROWS.
 * vgan_kpca_row_means: mean[r] (float64 [rows]) of every row of R [rows, m] (rows = count nq of a block): 64 partial sums,
 *   partial l over the columns l, l + 64, ... ascending, combined by the xor butterfly (p_l += p_{l ^ o} for o = 32, 16, 8, 4,
 *   2, 1), then divided by m.
 * vgan_kpca_scores: score[score_row[z] (or z), i] = float32(max(pot_i - proj_i, 0)) for the rows of R [count, rows, m] with
 *   row_mean [count, rows]: z_c = ((R[z][i][c] - row_mean_i) - col_mean_c) + total, y_j = sum_c V[j][c] z_c on the f64 matrix unit
 *   (c ascending), proj = sum_j wt_j y_j^2 in vgan_pca_scores' order and with its skip rules (they depend on wt alone), pot =
 *   (1 - 2 row_mean_i) + total.  col_mean, wt (float64 [S, m]), total (float64 [S]) and V (float64 [S, m, m], row j = component
 *   j) are indexed by first + z.  ld_score >= rows.
 * Every sum has one order: the bits of an element do not depend on the launch, the chunk or splits.  Every entry returns
 * VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_KPCA_MAX_LANDMARKS 1024
int vgan_kpca_center(const float* K, int m, int count, double* col_mean, double* total, double* Kc, vgan_stream_t stream);
int vgan_kpca_kernel_rows(const float* Pq, const float* sq_q, int nq, const float* Pr, const float* sq_r, int m,
                          const int32_t* feat_off, const int64_t* col_off, int first, int count, const double* gamma, int engine,
                          int splits, float* R, vgan_stream_t stream);
int vgan_kpca_row_means(const float* R, int64_t rows, int m, double* mean, vgan_stream_t stream);
int vgan_kpca_scores(const float* R, int rows, int m, int first, int count, const double* row_mean, const double* col_mean,
                     const double* total, const double* V, const double* wt, float* score, const int32_t* score_row,
                     int64_t ld_score, vgan_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * HiCS subspace contrast (Keller, Mueller, Boehm, ICDE 2012): the Monte-Carlo contrast of a feature set, the mean over M
 * draws of the Kolmogorov-Smirnov distance between one feature's sample conditioned on index slices of the others and its
 * full sample, taken on sort positions in integers (v-gan_amd/hics.py: subspace_contrast and HiCS, whose docstrings are the
 * definition; kernels in csrc/outlier_hics.hip).  2 <= n <= VGAN_HICS_MAX_ROWS: the two n-bit maps of a draw are 64 KB of LDS.
 * vgan_hics_argsort_columns: order, rank uint32 [d, n].  order[f, r] = the row at position r of the stable ascending sort
 *   of column f of X [n, d] (ldx), -0.0 taken as +0.0, ties to the lower row; rank[f, order[f, r]] = r.  A bitonic network
 *   on the 64-bit keys (orderable float bits << 32) | row, which are distinct, so the result is the unique stable order
 *   and NaN input cannot change a trip count.  keys: workspace uint64 [d, n_pad], n_pad the power of two with n <= n_pad
 *   < 2 n; runs of VGAN_HICS_SORT_RUN keys are sorted in LDS.
 * vgan_hics_contrast: subspace z (0 <= z < S) has the features feat[feat_off[z] .. feat_off[z + 1]) (ascending, k of them),
 *   the slice width width[z] (1 <= w <= n, computed by the host) and the stream id stream_id[z].  Draw t (0 <= t < M) uses
 *   the Philox4x32-10 words with key k0 = lo32(seed) ^ lo32(id), k1 = hi32(seed) ^ hi32(id) ^ 0x5bd1e995 and counter (t, q,
 *   VGAN_HICS_PHILOX_TAG, 0): c = (word 0 of q = 0 * k) >> 32 is the comparison position, start_p = (word p & 3 of q = 1 +
 *   (p >> 2) * (n - w + 1)) >> 32 the slice start of position p != c.  C = the rows that lie in order[f_p, start_p ..
 *   start_p + w) for every p != c, m = |C|, cnt(r) = #{rows of C with rank[f_c, .] < r},
 *       D = max over r = 1 .. n of |cnt(r) n - r m|                                            (64-bit integers).
 *   D int64, m and c int32 [S, M] receive every draw.  contrast[z] (float64) = (sum over t ascending of float64(D) /
 *   float64(n m), 0 where m = 0) / M; n_empty[z] (int32) counts the draws with m = 0.  k < 2: no draw is made, D = m = 0,
 *   c = -1, contrast 0, n_empty 0.  The membership of a draw is a bitmap in LDS indexed by rank[f_c, .]; with 2 w > n the
 *   complement of each slice is cleared from a full map instead, which gives the same set.  group: draws of one subspace
 *   that share a workgroup of 256 threads, 1 (a workgroup per draw) or VGAN_HICS_WAVE_GROUP (a wave per draw, n <=
 *   VGAN_HICS_WAVE_GROUP_MAX_ROWS), 0 = the library's choice; the results do not depend on it.  S * ceil(M / group) < 2^31.
 * Every entry returns VGAN_ERR_ARG before touching the device when an argument is out of range.
 * ------------------------------------------------------------------------------------------- */
#define VGAN_HICS_MAX_ROWS 262144 /* 2^18 */
#define VGAN_HICS_SORT_RUN 2048
#define VGAN_HICS_PHILOX_TAG 0x48494353u
#define VGAN_HICS_WAVE_GROUP 4
#define VGAN_HICS_WAVE_GROUP_MAX_ROWS 65536
int vgan_hics_argsort_columns(const float* X, int ldx, int n, int d, uint64_t* keys, int64_t n_pad, uint32_t* order,
                              uint32_t* rank, vgan_stream_t stream);
int vgan_hics_contrast(const uint32_t* order, const uint32_t* rank, int n, int d, const int32_t* feat, const int32_t* feat_off,
                       const int32_t* width, const uint64_t* stream_id, int S, int M, uint64_t seed, int group, int64_t* D,
                       int32_t* m, int32_t* c, double* contrast, int32_t* n_empty, vgan_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VGAN_HIP_H */

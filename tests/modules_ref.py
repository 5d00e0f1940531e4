"""TEST INFRASTRUCTURE ONLY: float64 restatements of what vgan_amd/modules.py computes at the operator boundary -- the Linear
chains through _LinearFn, the upper_softmax module, RBF.forward / _RBFMatrixFn and MMDLossConstrained on equal and unequal row
counts -- with first-order error bounds, the case tables of tests/test_modules_gpu.py, the drivers that run the real modules on
any device, and the check functions both tiers share.  tests/test_modules_cpu.py pins all of it without a GPU (the modules run
over tests/cpu_ops.CpuOps there).  The product never imports this file, and nothing below calls a kernel to form a reference.

Reused, not copied: gemm_ref (product_bound, cap_ok, worst_ratio, VARIANTS, ld_for, shift_for), mmd_ref (l_bound, backward_ref,
backward_bound, sum_bound, cap_ok, multipliers, scales, C_EPI, U) and small_ops_ref (softmax64, upper_mask_ref,
mask_backward_ref, colkey_ref, colkey_rows).

References
----------
rbf_matrix_ref   ONE N x N block: L_ij = max(s_i + s_j - 2 z_i . z_j, 0) from the norms s the kernel is GIVEN (mmd_ref's
                 convention), K = sum_k exp(-L / sc_k), dK/dL = -sum_k exp(-L / sc_k) / sc_k, sc_k = float32(bw) * float32(mult_k).
mmd_loss_ref     loss = mean(K_xx) - 2 mean(K_xy) + mean(K_yy) + weight * mean_j(1 - max_i U_ij) with block means over n_x^2,
                 n_x n_y and n_y^2 entries (equal and unequal rows alike); dZ_i = 2 sum_j W_ij (z_i - z_j), W = (gK + gK^T) * dK/dL
                 with the block-constant gK; dU = -weight / d on the arg-max row of each column, the LOWEST row on ties
                 (small_ops_ref.colkey_ref is the rule).
chain_ref        per Linear layer y = x W^T + b, dx = dy W, dW = dy^T x, db = column sums of dy, in float64 on that layer's OWN
                 device inputs, so that every product is held to its own gemm_ref.product_bound and nothing compounds.

Bounds (u = 2^-24; first order, order independent, none fitted to a device)
--------------------------------------------------------------------------
dL_ij   mmd_ref.l_bound with kterms = the padded p (the contraction the kernels run), plus, where the MODULE forms the norms
        (ops.row_sqnorm; the test cannot see them), 2 pp u (s_i + s_j): a float32 sum of pp squares in any order, doubled.
K_ij    |dK/dL| dL + C_EPI u K + n_kernels 2^-126          (the dK_ij form of mmd_ref's docstring)
dK_ij   sum_k exp(-L / sc_k) / sc_k^2 dL + C_EPI u |dK/dL| + 2^-126 sum_k 1 / sc_k      (its dw_ij form without 2 / n^2)
        The 2^-126 terms are the float32 format's own: an exponential below the smallest normal number may come back as zero.
Z.grad  mmd_ref.backward_bound(W, ...) over N columns plus 2 sum_j dW_ij |z_ik - z_jk|, dW_ij = |gK_ij + gK_ji| bound(dK_ij)
        + 4u |W_ij| (the float32 sum gK + gK^T and its product with dK/dL, doubled); times |gl| plus 2u |grad| for the product
        with the upstream scale.
loss    equal rows: sum of mmd_ref.sum_bound over the tile table (TWICE tiles doubled, XY doubled) / n^2; unequal rows: the
        per-element K bounds summed per block / the block's count (the row dots and their sum are float64) plus u |mean| per
        block, because the three means pass through a float32 buffer (`sums` of _MMDLossUnequalFn.forward) on their way to
        vgan_mmd_loss; both: the norm term of dL carried through |dK/dL|, and 8u (|xx| + 2 |xy| + |yy| + |weight pen|).
bw      sum_bound(..., calibrate=True) over the table / (N^2 - N), the norm term, and u bw for the float32 store.
chain   gemm_ref.product_bound per product; forward (K + 1) 2u (|x| |W|^T + |b|); db n 2u sum |dy|.
softmax S within 2u (3 |t_j| + 3 + sum_k S_k (3 |t_k| + 2) + d) S_j + 2^-126 of float64, t = x - max: the subtraction, the
        product with log2(e) and v_exp_f32 per term (3 |t| + 2), the same weighted over the denominator, d for a float32 sum of d
        positive terms in any order, one division; doubled.  Backward s_j (gs_j - A): 2 d u s_j sum_k |gs_k s_k| for the sum
        and 4u s_j (|gs_j| + sum_k |gs_k s_k|) for the difference and the product.

A vacuous bound hides errors: every case asserts mmd_ref.cap_ok (CAP_FP32 = 2e-4 of max |K|, of max |dK/dL|) or gemm_ref.cap_ok
(CAP = 2e-2 of max |want|, every product and every gradient) BEFORE a device result is looked at, and the CPU tier proves each
listed case inside its cap from the reference alone.

One case had to change to keep a cap.  The bandwidth 1e-3 times the calibrated one cannot stay inside CAP_FP32: on the diagonal
(and on a planted duplicate) L is s_i + s_i - 2 g_ii, a cancellation whose honest error is dL = (4 pp + 16) u s_i, and K moves by
dL / sc of its value; with sc a thousandth of bw ~ 2 s that is (4 pp + 16) u 500 / min(mult) -- 1.3e-3 to 0.7 of K over the cases
of the table (the CPU tier's figures), against a cap of 2e-4, whatever the data's scale (dL and sc scale alike), and a bandwidth at which the
off-diagonal underflows (L / sc > 104) is always at least 25 times past the cap.  Those launches are kept, as the property they
are there for: K and dK/dL finite everywhere, every element whose float64 value is below 2^-160 exactly zero, K the same bits
with and without dK, nothing written outside [m, m) -- and err <= bound is still asserted per element (off the diagonal the
bound is about n_kernels 2^-126 there, which is sharp); only cap_ok is not asserted for that factor.  Every other case keeps
both caps as stated.
"""
import types
import zlib

import numpy as np
import torch

import gemm_ref as gr
import mmd_ref as mr
import small_ops_ref as sr
from gemm_ref import VARIANTS, ld_for, product_bound, shift_for, worst_ratio  # noqa: F401  (the GPU tier takes them from here)
from mmd_ref import C_EPI, CAP_FP32, U, backward_bound, backward_ref, l_bound, multipliers, scales, sum_bound

TINY = 2.0 ** -126
CAP = gr.CAP
FAMILIES = ["chain fwd", "chain dx", "chain dW", "chain db", "softmax fwd", "softmax bwd", "K", "dK", "Z.grad", "loss", "loss grad"]


class Case(types.SimpleNamespace):
    pass


def round4(v):
    return (int(v) + 3) // 4 * 4


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def ratio_of(got, want, bound):
    """gemm_ref.worst_ratio: err <= bound element-wise, returns max err / bound"""
    return worst_ratio(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64))


# =============================================================================================== case tables
CHAIN_SHAPES = [(1, 1, 5), (5, 3, 7), (63, 3, 20), (65, 5, 67), (130, 5, 36)]  # (n, L, d): widths 2/4/8, 6/12/24, 10/20/40
CHAIN_KINDS = ["gen", "enc", "dec", "det"]
CHAIN_MODES = ["all", "x frozen", "weight frozen", "bias frozen", "sum"]  # what requires grad; "sum": dy from .sum().backward()
SOFTMAX_SHAPES = [(1, 1), (3, 5), (65, 64), (5, 260)]
KERNELS = [(1, 2.0), (5, 2.0), (3, 3.0), (8, 1.5)]
BW_FACTORS = [1.0, 1e-3, 1e3]
RBF_M = [1, 2, 63, 64, 65, 129]
RBF_P = [1, 3, 4, 31, 32, 33, 36, 68]
RBF_DIRECT = [(m, p) for m in RBF_M for p in (3, 36)] + [(65, p) for p in RBF_P if p not in (3, 36)]
RBF_MODULE_N = [2, 63, 64, 65, 129]
RBF_MODULE_P = [1, 3, 4, 5, 33]
RBF_MODULE = [(N, 4) for N in RBF_MODULE_N] + [(64, p) for p in RBF_MODULE_P if p != 4] + [(65, 33), (129, 5)]
EQUAL_CASES = [(2, 3, 5), (33, 5, 9), (64, 4, 4), (65, 33, 4), (100, 20, 20)]  # (n, p, d)
LOSS_KERNELS = [(5, 2.0), (3, 3.0), (8, 1.5)]
UNEQUAL_CASES = [(1, 3, 2, 2, 3), (33, 70, 12, 5, 7), (64, 2, 64, 4, 4), (70, 131, 70, 3, 3)]  # (n_x, n_y, rows of U, p, d)
NEEDS = [(True, False), (False, True), (True, True), (False, False)]  # gradient wanted for (X, Y)
GL = 2.5
WEIGHT = 3.0


def direct_plan(index):
    """(variant, (n_kernels, mul_factor), bandwidth factor) of the launches of one direct case: every kernel setting on the
    aligned layout at the calibrated bandwidth, the default kernel there at the two other bandwidths, and on each of the two
    scalar layouts one setting (rotating with the case) at all three bandwidths."""
    plan = [("aligned", k, 1.0) for k in KERNELS] + [("aligned", (5, 2.0), f) for f in BW_FACTORS[1:]]
    for v, variant in enumerate(VARIANTS[1:]):
        plan += [(variant, KERNELS[(index + v) % len(KERNELS)], f) for f in BW_FACTORS]
    return plan


# =============================================================================================== RBF matrix
def rbf_operand(m, p, name, duplicates=True):
    """Z [m, p] float32 standard normal with a planted pair of duplicate rows (m >= 3), the float32 norms and the calibrated
    bandwidth (m = 1 leaves no pair to calibrate from: twice the norm, what independent rows of that size would give)."""
    rng = rng_for(f"rbf/{name}/{m}/{p}")
    Z = rng.normal(size=(m, p)).astype(np.float32)
    if duplicates and m >= 3:
        Z[m - 1] = Z[m // 2]
    z64 = Z.astype(np.float64)
    sq = (z64 * z64).sum(1).astype(np.float32)
    s = sq.astype(np.float64)
    L = np.maximum(s[:, None] + s[None, :] - 2.0 * z64 @ z64.T, 0.0)
    bw = np.float32(L.sum() / (m * m - m)) if m > 1 else np.float32(2.0 * s[0])
    return Z, sq, bw


def rbf_matrix_ref(z64, sq64, bw32, mults, norm_terms=0):
    """L, K, dK = dK/dL of ONE block and their bounds bK, bdK (module docstring).  z64: the operand the kernel contracts (the
    padded one, for the module), sq64: the float32 norms widened, norm_terms: pp where the module forms the norms itself."""
    z64 = np.asarray(z64, dtype=np.float64)
    s = np.asarray(sq64, dtype=np.float64)
    L = np.maximum(s[:, None] + s[None, :] - 2.0 * (z64 @ z64.T), 0.0)
    sc = scales(bw32, list(mults))
    K, dK, s2 = np.zeros_like(L), np.zeros_like(L), np.zeros_like(L)
    for c in sc:
        e = np.exp(-L / c)
        K += e
        dK -= e / c
        s2 += e / c ** 2
    dL = l_bound(z64, s, L, z64.shape[1]) + 2.0 * norm_terms * U * (s[:, None] + s[None, :])
    bK = -dK * dL + C_EPI * U * K + len(sc) * TINY
    bdK = s2 * dL + C_EPI * U * -dK + TINY * float((1.0 / sc).sum())
    return Case(L=L, K=K, dK=dK, bK=bK, bdK=bdK, dL=dL, sc=sc)


def rbf_single_ref(z64, sq64, alpha):
    """vgan_rbf_kernel_matrix: exp(-alpha L) off the diagonal (one scale 1 / alpha), exactly 1 on it."""
    r = rbf_matrix_ref(z64, sq64, np.float32(1.0), [1.0 / float(np.float32(alpha))])
    np.fill_diagonal(r.K, 1.0)
    return r


def underflown(r):
    """elements whose float64 K is below 2^-160 even with L at the near end of its error interval: exactly zero in float32"""
    near = np.maximum(r.L - r.dL, 0.0)
    return sum(np.exp(-near / c) * max(1.0, 1.0 / c) for c in r.sc) < 2.0 ** -160


def pair_term(dW, z64):
    """2 sum_j dW_ij |z_ik - z_jk|"""
    out = np.zeros_like(z64)
    for k in range(z64.shape[1]):
        out[:, k] = 2.0 * (dW * np.abs(z64[:, None, k] - z64[None, :, k])).sum(1)
    return out


def pad_rows(*blocks):
    """[X; Y; ...] zero-padded to a multiple of 4 columns, as the modules stage it"""
    Z = np.vstack(blocks).astype(np.float32)
    out = np.zeros((Z.shape[0], round4(Z.shape[1])), dtype=np.float32)
    out[:, :Z.shape[1]] = Z
    return out


def given_norms(Zp):
    z64 = Zp.astype(np.float64)
    return z64, (z64 * z64).sum(1).astype(np.float32).astype(np.float64)


def whole_table(tiles_of, N):
    """the tile table _device_bandwidth sums the pair distances over: the XX tiles of the N-row table"""
    t = np.asarray(tiles_of(N, 0))
    return t[(t[:, 4] & 3) == 0]


def bandwidth_ref(z64, sq64, table, n):
    """float64 calibrated bandwidth sum(L) / (N^2 - N) and its bound (module docstring, bw).  table: the tiles the module sums
    over -- the n-row table of the equal path, or whole_table(N) with n = N."""
    N, pp = z64.shape
    s = sq64
    L = np.maximum(s[:, None] + s[None, :] - 2.0 * (z64 @ z64.T), 0.0)
    want = L.sum() / (float(N) * N - N)
    per = sum_bound(table, z64, sq64, n, 1.0, pp, 64, calibrate=True)
    tot = mr.reduce_stats(table, np.zeros(len(table)), per)[3]
    norm = 2.0 * pp * U * 2.0 * N * s.sum()
    return want, (tot + norm) / (float(N) * N - N) + 2.0 * U * want


def rbf_module_ref(Z, G, bw32, kernel):
    """RBF.forward(Z) and the gradient of sum(K * G) to Z, on the padded operand, with bounds; bw32: the bandwidth in use."""
    Zp = pad_rows(Z)
    z64, sq64 = given_norms(Zp)
    N, pp = Zp.shape
    r = rbf_matrix_ref(z64, sq64, bw32, multipliers(*kernel), norm_terms=pp)
    g = np.asarray(G, dtype=np.float64)
    gs = g + g.T
    W = gs * r.dK
    dW = np.abs(gs) * r.bdK + 4.0 * U * np.abs(W)
    r.W, r.Zp, r.z64, r.sq64 = W, Zp, z64, sq64
    r.dZ = backward_ref(W, z64, 0, N)[:, :Z.shape[1]]
    r.bdZ = (backward_bound(W, z64, 0, N, N) + pair_term(dW, z64))[:, :Z.shape[1]]
    return r


def mmd_loss_ref(X, Y, Um, weight, bw32, kernel, gl=1.0, tiles_of=None):
    """MMDLossConstrained in float64 (module docstring) with bounds.  kernel = (n_kernels, mul_factor); tiles_of(n, grad_mode):
    the library's tile table, needed for the equal-row loss bound only."""
    nx, p = X.shape
    ny, d = Y.shape[0], Um.shape[1]
    N, pp = nx + ny, round4(p)
    Zp = pad_rows(X, Y)
    z64, sq64 = given_norms(Zp)
    mults = multipliers(*kernel)
    r = rbf_matrix_ref(z64, sq64, bw32, mults, norm_terms=pp)
    blocks = [(slice(0, nx), slice(0, nx), 1.0), (slice(0, nx), slice(nx, N), -2.0), (slice(nx, N), slice(nx, N), 1.0)]
    gK = np.zeros((N, N))
    means, mean_bounds, norm_part = [], [], 0.0
    for ri, cj, coef in blocks:
        cnt = float(ri.stop - ri.start) * (cj.stop - cj.start)
        gK[ri, cj] = coef / cnt
        means.append(r.K[ri, cj].sum() / cnt)
        mean_bounds.append(r.bK[ri, cj].sum() / cnt)
        norm_part += abs(coef) * (-r.dK[ri, cj] * 2.0 * pp * U * (sq64[ri, None] + sq64[None, cj])).sum() / cnt
    xx, xy, yy = means
    u32 = np.asarray(Um, dtype=np.float32)
    keys = sr.colkey_ref(u32, 0)
    rows = sr.colkey_rows(keys)
    colmax = u32[rows, np.arange(d)].astype(np.float64)
    assert np.array_equal(colmax, u32.max(0).astype(np.float64))
    pen = float(weight) * float(np.mean(1.0 - colmax))
    loss = xx - 2.0 * xy + yy + pen
    equal = nx == ny and Um.shape[0] == nx
    if equal:
        table = np.asarray(tiles_of(nx, 0))
        per = sum_bound(table, z64, sq64, nx, bw32, pp, 64, None if kernel == (5, 2.0) else mults)
        st = mr.reduce_stats(table, per)
        sums = (st[0] + 2.0 * st[1] + st[2]) / (float(nx) * nx) + norm_part
    else:
        sums = mean_bounds[0] + 2.0 * mean_bounds[1] + mean_bounds[2] + U * (abs(xx) + 2.0 * abs(xy) + abs(yy))
    bloss = sums + 8.0 * U * (abs(xx) + 2.0 * abs(xy) + abs(yy) + abs(pen))
    gs = gK + gK.T
    W = gs * r.dK
    dW = np.abs(gs) * r.bdK + 4.0 * U * np.abs(W)
    dZ = backward_ref(W, z64, 0, N) * gl
    bdZ = (backward_bound(W, z64, 0, N, N) + pair_term(dW, z64)) * abs(gl) + 2.0 * U * np.abs(dZ)
    dU = np.zeros((Um.shape[0], d))
    dU[rows, np.arange(d)] = -float(weight) / d * gl
    return Case(loss=loss, bloss=bloss, xx=xx, xy=xy, yy=yy, pen=pen, dX=dZ[:nx, :p], dY=dZ[nx:, :p], bdX=bdZ[:nx, :p], bdY=bdZ[nx:, :p],
                dU=dU, bdU=4.0 * U * np.abs(dU), rows=rows, r=r, W=W, z64=z64, sq64=sq64, N=N, pp=pp, nx=nx)


def loss_caps(ref):
    """every cap of one loss case, from the reference alone; returns the ratios"""
    out = dict(K=mr.cap_ok(ref.r.bK, ref.r.K, CAP_FP32), dK=mr.cap_ok(ref.r.bdK, ref.r.dK, CAP_FP32))
    out["dX"], out["dY"] = gr.cap_ok(ref.bdX, ref.dX), gr.cap_ok(ref.bdY, ref.dY)
    return out


def loss_data(name, nx, ny, nu, p, d, ties=False):
    """X standard normal, Y = rows of X (cycled) * U(0.2, 1); U uniform in (0.01, 1) with unique column maxima, or (ties) the
    upper_softmax of random logits: many entries exactly 1."""
    rng = rng_for(f"loss/{name}/{nx}/{ny}/{nu}/{p}/{d}")
    X = rng.normal(size=(nx, p)).astype(np.float32)
    Y = (X[np.arange(ny) % nx] * rng.uniform(0.2, 1.0, size=(ny, p)) + (0.0 if ny == nx else 0.1 * rng.normal(size=(ny, p)))).astype(np.float32)
    if ties:
        Um = sr.upper_mask_ref(sr.softmax64(rng.normal(size=(nu, d)) * 2.0).astype(np.float32))
    else:
        Um = rng.uniform(0.01, 1.0, size=(nu, d)).astype(np.float32)
        assert all((Um[:, j] == Um[:, j].max()).sum() == 1 for j in range(d))
    return X, Y, Um


# =============================================================================================== drivers (any device)
def to_dev(a, device, grad=False):
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    return t.requires_grad_(True) if grad else t


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def run_loss(M, X, Y, Um, kernel, need, device, u_grad=False, gl=None, bandwidth=None, loss_fn=None, weight=WEIGHT):
    """One forward (and backward, where anything requires grad) of the real MMDLossConstrained.  Returns the float32 loss, the
    bandwidth in use, the gradients (None where none arrived), and the graph's pieces for a second backward."""
    if loss_fn is None:
        loss_fn = M.MMDLossConstrained(weight, M.RBF(kernel[0], kernel[1], bandwidth))
    Xt, Yt, Ut = to_dev(X, device, need[0]), to_dev(Y, device, need[1]), to_dev(Um, device, u_grad)
    loss = loss_fn(Xt, Yt, Ut)
    out = Case(loss=float(loss.detach()), loss_t=loss, loss_fn=loss_fn, bw=float(loss_fn.bandwidth), Xt=Xt, Yt=Yt, Ut=Ut,
               requires_grad=loss.requires_grad)
    if loss.requires_grad:
        (loss if gl is None else loss * gl).backward(retain_graph=True)
    out.dX, out.dY, out.dU = host(Xt.grad), host(Yt.grad), host(Ut.grad)
    return out


def check_loss(got, ref, need, u_grad, worst=None):
    """The checks of the GPU tier on one loss case: the loss and every gradient within its bound, a gradient exactly where the
    reference's autograd would leave one.  Returns {family: ratio}."""
    rec = {"loss": ratio_of(got.loss, ref.loss, ref.bloss)}
    assert got.requires_grad == (need[0] or need[1] or u_grad)
    g = 0.0
    for have, val, want, bound, name in ((need[0], got.dX, ref.dX, ref.bdX, "dX"), (need[1], got.dY, ref.dY, ref.bdY, "dY"),
                                         (u_grad, got.dU, ref.dU, ref.bdU, "dU")):
        assert (val is not None) == bool(have), f"{name}: a gradient where none is due, or none where one is"
        if have:
            assert val.shape == want.shape, name
            g = max(g, ratio_of(val, want, bound))
    if need[0] or need[1] or u_grad:
        rec["loss grad"] = g
    if worst is not None:
        for k, v in rec.items():
            worst[k] = max(worst[k], v)
    return rec


def run_rbf(M, ops, Z, G, kernel, device, bandwidth=None, k=None):
    """RBF.forward on Z with gradient of sum(K * G) to Z; G is handed over as a transposed (non-contiguous) view.  Also the
    direct ops.rbf_multi_kernel_matrix call on the padded operand at the bandwidth the module used."""
    k = M.RBF(kernel[0], kernel[1], bandwidth) if k is None else k
    Zt = to_dev(Z, device, True)
    K = k(Zt)
    Gt = to_dev(np.ascontiguousarray(np.asarray(G, dtype=np.float32).T), device).t()
    assert not Gt.is_contiguous() or Gt.shape[0] == 1
    (K * Gt).sum().backward(retain_graph=True)
    bw = float(k.bandwidth)
    Zp = to_dev(pad_rows(Z), device)
    sq = torch.empty(Zp.shape[0], dtype=torch.float32, device=device)
    ops.row_sqnorm(Zp, sq, Zp.shape[1])
    Kd = torch.empty(Zp.shape[0], Zp.shape[0], dtype=torch.float32, device=device)
    ops.rbf_multi_kernel_matrix(Zp, sq, torch.as_tensor([bw], dtype=torch.float32, device=device), k.bandwidth_multipliers.tolist(), Kd, None)
    return Case(K=host(K), K_t=K, Gt=Gt, Zt=Zt, dZ=host(Zt.grad), bw=bw, k=k, K_direct=host(Kd))


def check_rbf(got, ref, worst=None):
    rec = {"K": ratio_of(got.K, ref.K, ref.bK), "Z.grad": ratio_of(got.dZ, ref.dZ, ref.bdZ)}
    assert np.array_equal(got.K.view(np.uint32), got.K_direct.view(np.uint32)), "RBF.forward differs from the direct kernel call"
    if worst is not None:
        for k, v in rec.items():
            worst[k] = max(worst[k], v)
    return rec


# ---- Linear chains
def chain_module(M, kind, L, d):
    """the module of a kind with seeded parameters (nn.Linear's own initialisation under a fixed seed) and its input width"""
    torch.manual_seed(zlib.crc32(f"{kind}/{L}/{d}".encode()) & 0x7FFFFFFF)
    if kind == "gen":
        return M.Generator_big(L, d), L
    if kind == "enc":
        return M.Encoder(L, d), d
    if kind == "dec":
        return M.Decoder(L, d), L
    return M.Detector(L, d, M.Encoder, M.Decoder), d


def chain_layers(mod, kind):
    mains = [mod.encoder.main, mod.decoder.main] if kind == "det" else [mod.main]
    return [m for main in mains for m in main if isinstance(m, torch.nn.Linear)]


def chain_outputs(kind, out):
    return list(out) if kind == "det" else [out]


def apply_mode(layers, mode):
    """which tensors require grad: layer 1's weight or bias is frozen in the two 'frozen' modes"""
    for m in layers:
        m.weight.requires_grad_(True), m.bias.requires_grad_(True)
    if mode == "weight frozen":
        layers[1].weight.requires_grad_(False)
    if mode == "bias frozen":
        layers[1].bias.requires_grad_(False)


def run_chain(M, kind, n, L, d, mode, device):
    """The module's forward and backward, then the same chain by hand from hip_linear calls with retain_grad() on every
    intermediate.  Returns the per-layer records of the hand-built chain and the two results to compare bit for bit."""
    mod, width = chain_module(M, kind, L, d)
    mod = mod.to(device)
    layers = chain_layers(mod, kind)
    apply_mode(layers, mode)
    rng = rng_for(f"chain/{kind}/{n}/{L}/{d}")
    x = rng.normal(size=(n, width)).astype(np.float32)
    x_grad = mode != "x frozen"
    params = [q for m in layers for q in (m.weight, m.bias)]

    def backward(outs, Gs):
        if mode == "sum":
            sum(o.sum() for o in outs).backward()  # dy is an expanded scalar: a non-contiguous (stride 0) tensor
        else:
            sum((o * g).sum() for o, g in zip(outs, Gs)).backward()

    xt = to_dev(x, device, x_grad)
    outs = chain_outputs(kind, mod(xt))
    Gs = [to_dev(rng.normal(size=tuple(o.shape)), device) for o in outs]
    backward(outs, Gs)
    first = Case(outs=[host(o) for o in outs], grads=[host(q.grad) for q in params], dx=host(xt.grad))
    for q in params:
        q.grad = None
    xh = to_dev(x, device, x_grad)
    hs, h = [xh], xh
    for i, m in enumerate(layers):
        h = M.hip_linear(h, m)
        if h.requires_grad:
            h.retain_grad()
        hs.append(h)
    if kind == "gen":
        outs2 = [mod.main[-1](h)]
    elif kind == "det":
        outs2 = [hs[4].view(n, -1), hs[8].view(n, -1)]
    else:
        outs2 = [h]
    backward(outs2, Gs)
    second = Case(outs=[host(o) for o in outs2], grads=[host(q.grad) for q in params], dx=host(xh.grad))
    recs = []
    for i, m in enumerate(layers):
        extra = host(Gs[0]) if (kind == "det" and i == 4 and mode != "sum") else (np.ones((n, L), dtype=np.float32) if (kind == "det" and i == 4) else None)
        recs.append(Case(x=host(hs[i]), W=host(m.weight), b=host(m.bias), y=host(hs[i + 1]), dy=host(hs[i + 1].grad), dx=host(hs[i].grad),
                         dW=host(m.weight.grad), db=host(m.bias.grad), extra=extra, needs=(hs[i].requires_grad, m.weight.requires_grad, m.bias.requires_grad)))
    return Case(first=first, second=second, recs=recs, x_grad=x_grad)


def run_nobias(M, n, kin, out, device):
    """hip_linear on nn.Linear(bias=False): (y, dx, dW) from the device, their float64 values and product bounds"""
    torch.manual_seed(zlib.crc32(f"nobias/{n}/{kin}/{out}".encode()) & 0x7FFFFFFF)
    layer = torch.nn.Linear(kin, out, bias=False).to(device)
    rng = rng_for(f"nobias/{n}/{kin}/{out}")
    x, G = rng.normal(size=(n, kin)).astype(np.float32), rng.normal(size=(n, out)).astype(np.float32)
    xt = to_dev(x, device, True)
    y = M.hip_linear(xt, layer)
    (y * to_dev(G, device)).sum().backward()
    assert layer.bias is None
    x64, g64, w64 = x.astype(np.float64), G.astype(np.float64), host(layer.weight).astype(np.float64)
    return ([host(y), host(xt.grad), host(layer.weight.grad)], [x64 @ w64.T, g64 @ w64, g64.T @ x64],
            [product_bound(x64, w64.T, kin), product_bound(g64, w64, out), product_bound(g64.T, x64, n)])


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def chain_ref(rec):
    """float64 y, dx, dW, db of ONE layer from its own device inputs, each with its product bound.  `extra`: a gradient that
    reaches the layer's INPUT directly as well (the Detector's enc output): the input's grad is extra + dy W, one more rounding."""
    x, W, b, dy = (np.asarray(a, dtype=np.float64) for a in (rec.x, rec.W, rec.b, rec.dy))
    n, kin = x.shape
    out = W.shape[0]
    r = Case(y=x @ W.T + b, by=(kin + 1) * 2.0 * U * (np.abs(x) @ np.abs(W).T + np.abs(b)),
             dx=dy @ W, bdx=product_bound(dy, W, out), dW=dy.T @ x, bdW=product_bound(dy.T, x, n),
             db=dy.sum(0), bdb=n * 2.0 * U * np.abs(dy).sum(0))
    if rec.extra is not None:
        e = np.asarray(rec.extra, dtype=np.float64)
        r.bdx = r.bdx + 2.0 * U * (np.abs(e) + np.abs(r.dx))
        r.dx = r.dx + e
    return r


def chain_caps(recs):
    for rec in recs:
        r = chain_ref(rec)
        for want, bound in ((r.y, r.by), (r.dx, r.bdx), (r.dW, r.bdW), (r.db, r.bdb)):
            gr.cap_ok(bound, want)


def check_chain(run, worst=None):
    """The checks of the GPU tier on one chain: module == hand-built chain bit for bit (outputs, every parameter gradient, the
    input's gradient); a gradient exactly where one is due; every layer's y, dx, dW, db within its product bound."""
    a, b = run.first, run.second
    assert all(same_bits(p, q) for p, q in zip(a.outs, b.outs)), "the module's output differs from the hand-built chain"
    assert all(same_bits(p, q) for p, q in zip(a.grads, b.grads)), "a parameter gradient differs from the hand-built chain"
    assert same_bits(a.dx, b.dx) and (a.dx is not None) == run.x_grad
    rec_out = {"chain fwd": 0.0, "chain dx": 0.0, "chain dW": 0.0, "chain db": 0.0}
    for i, rec in enumerate(run.recs):
        r = chain_ref(rec)
        rec_out["chain fwd"] = max(rec_out["chain fwd"], ratio_of(rec.y, r.y, r.by))
        for have, got, want, bound, fam in ((rec.needs[0], rec.dx, r.dx, r.bdx, "chain dx"), (rec.needs[1], rec.dW, r.dW, r.bdW, "chain dW"),
                                            (rec.needs[2], rec.db, r.db, r.bdb, "chain db")):
            assert (got is not None) == bool(have), f"layer {i} {fam}: a gradient where none is due, or none where one is"
            if have:
                rec_out[fam] = max(rec_out[fam], ratio_of(got, want, bound))
    if worst is not None:
        for k, v in rec_out.items():
            worst[k] = max(worst[k], v)
    return rec_out


# ---- upper_softmax
SNAP_MARGIN = 1e-5


def softmax_logits(n, d):
    """random logits (spread 2) with no float64 softmax entry within 1e-5 / d of the snap threshold 1 / d (redrawn per element
    until that holds); n >= 3: row 1 is a 200-wide spread, as edge_logits of test_small_ops_gpu.py"""
    rng = rng_for(f"softmax/{n}/{d}")
    x = (rng.normal(size=(n, d)) * 2.0).astype(np.float32)
    if n >= 3:
        x[1] = np.linspace(-100.0, 100.0, d, dtype=np.float32)
    for _ in range(100):
        near = np.abs(sr.softmax64(x) - 1.0 / d) < SNAP_MARGIN / d
        if not near.any() or d == 1:
            break
        x[near] += np.float32(0.37)
    return x


def snap_clear(x):
    d = x.shape[1]
    return d == 1 or not (np.abs(sr.softmax64(x) - 1.0 / d) < SNAP_MARGIN / d).any()


def softmax_bound(x):
    x64 = np.asarray(x, dtype=np.float64)
    S = sr.softmax64(x64)
    t = np.abs(x64 - x64.max(1, keepdims=True))
    d = x64.shape[1]
    return 2.0 * U * (3.0 * t + 3.0 + (S * (3.0 * t + 2.0)).sum(1, keepdims=True) + d) * S + TINY


def run_softmax(M, x, g, device):
    xt = to_dev(x, device, True)
    Ut = M.upper_softmax()(xt)
    (S,) = Ut.grad_fn.saved_tensors
    (Ut * to_dev(g, device)).sum().backward(retain_graph=True)
    return Case(U=host(Ut), S=host(S), dl=host(xt.grad), U_t=Ut, xt=xt)


def check_softmax(got, x, g, worst=None):
    d = x.shape[1]
    want = sr.softmax64(x)
    rec = {"softmax fwd": ratio_of(got.S, want, softmax_bound(x))}
    assert np.array_equal(got.U.view(np.uint32), sr.upper_mask_ref(got.S).view(np.uint32)), "U is not the mask of the saved S"
    assert np.array_equal(got.U == 1, want >= 1.0 / d), "a snap decision differs from float64 away from the threshold"
    s = got.S.astype(np.float64)
    wantb = sr.mask_backward_ref([g], got.S, None, 0.0, 0)
    gs = np.where(got.S < np.float32(1.0 / d), g.astype(np.float64), 0.0)
    A = np.abs(gs * s).sum(1, keepdims=True)
    bound = s * (2.0 * d * U * A + 4.0 * U * (np.abs(gs) + A)) + TINY
    rec["softmax bwd"] = ratio_of(got.dl, wantb, bound)
    if worst is not None:
        for k, v in rec.items():
            worst[k] = max(worst[k], v)
    return rec


# ---- repeat and isolation (both tiers)
def second_backward_of_the_loss(M, data, kernel, device):
    """A retained graph of MMDLossConstrained differentiated three times, and once per input: the same bits every time."""
    X, Y, Um = data
    got = run_loss(M, X, Y, Um, kernel, (True, True), device, u_grad=True)
    ins = [got.Xt, got.Yt, got.Ut]
    for _ in range(2):
        dX, dY, dU = (host(g) for g in torch.autograd.grad(got.loss_t, ins, retain_graph=True))
        assert same_bits(dX, got.dX) and same_bits(dY, got.dY) and same_bits(dU, got.dU)
    (dX,) = torch.autograd.grad(got.loss_t, [got.Xt], retain_graph=True)  # two separate calls, for X and for Y
    (dY,) = torch.autograd.grad(got.loss_t, [got.Yt], retain_graph=True)
    assert same_bits(host(dX), got.dX) and same_bits(host(dY), got.dY)


def second_backward_of_the_others(M, ops, device):
    """_RBFMatrixFn, _UpperSoftmaxFn and a Detector's chain of _LinearFn: a second backward on the retained graph, same bits."""
    Z, _, _ = rbf_operand(65, 5, "module")
    G = rng_for("G/65/5").normal(size=(65, 65)).astype(np.float32)
    got = run_rbf(M, ops, Z, G, (3, 3.0), device)
    (again,) = torch.autograd.grad((got.K_t * got.Gt).sum(), [got.Zt], retain_graph=True)
    assert same_bits(host(again), got.dZ)
    x = softmax_logits(65, 64)
    g = rng_for("g").normal(size=(65, 64)).astype(np.float32)
    sm = run_softmax(M, x, g, device)
    (again,) = torch.autograd.grad((sm.U_t * to_dev(g, device)).sum(), [sm.xt], retain_graph=True)
    assert same_bits(host(again), sm.dl)
    mod, width = chain_module(M, "det", 3, 20)
    mod = mod.to(device)
    xt = to_dev(rng_for("x").normal(size=(63, width)), device, True)
    enc, dec = mod(xt)
    loss = (enc * enc).sum() + dec.sum()
    params = list(mod.parameters())
    first = torch.autograd.grad(loss, [xt] + params, retain_graph=True)
    second = torch.autograd.grad(loss, [xt] + params, retain_graph=True)
    assert all(same_bits(host(a), host(b)) for a, b in zip(first, second))


def two_live_graphs(M, data, device):
    """Two graphs built from one loss_fn before either backward give the gradients of two graphs built and consumed in turn."""
    X, Y, Um = data
    X2, Y2 = (X * np.float32(0.7)).astype(np.float32), (Y * np.float32(1.2) + np.float32(0.05)).astype(np.float32)
    fn = M.MMDLossConstrained(WEIGHT, M.RBF(5, 2.0, 7.5))
    a = run_loss(M, X, Y, Um, None, (True, True), device, u_grad=True, loss_fn=fn)
    b = run_loss(M, X2, Y2, Um, None, (True, True), device, u_grad=True, loss_fn=fn)
    ins = [to_dev(v, device, True) for v in (X, Y, Um, X2, Y2, Um)]
    l1, l2 = fn(*ins[:3]), fn(*ins[3:])
    l2.backward()
    l1.backward()
    for t, want in zip(ins, (a.dX, a.dY, a.dU, b.dX, b.dY, b.dU)):
        assert same_bits(host(t.grad), want)
    assert float(l1.detach()) == a.loss and float(l2.detach()) == b.loss

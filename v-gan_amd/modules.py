"""Operator boundary: the reference's ``nn.Module`` classes with the same names, constructor
arguments, attributes and state_dict keys, whose forward/backward run on libvgan_hip.so.

  Generator_big, upper_softmax   <- src/models/Generator.py:6-22, 58-70
  Encoder, Decoder, Detector     <- src/models/Detector.py:5-48
  RBF, MMDLossConstrained        <- src/models/Mmd_loss_constrained.py:5-50

Tensors must live on a HIP device; there is no CPU path (HipOps raises).
"""
import torch
from torch import nn

from .ops import default_ops


def _round4(v):
    return (v + 3) // 4 * 4


def _dense(t):
    """Row-major with canonical strides.  ``contiguous()`` alone does not give that: it leaves the stride of a size-1 dimension as
    it is (the expanded scalar that ``.sum().backward()`` hands a [1, 1] output keeps stride 0), and the kernels take
    ``stride(0)`` as the leading dimension."""
    t = t.contiguous()
    if t.dim() == 2 and t.stride() != (t.shape[1], 1):
        t = torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)
    return t


class _LinearFn(torch.autograd.Function):
    """F.linear on the fp32 MFMA (vgan_linear_forward / _backward_input / _backward_params)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ops = default_ops()
        x = _dense(x)
        y = torch.empty(x.shape[0], W.shape[0], dtype=torch.float32, device=x.device)
        ops.linear_forward(x, W, b, y)
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        ops = default_ops()
        x, W = ctx.saved_tensors
        dy = _dense(dy)
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ops.linear_backward_input(dy, W, dx)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dW = torch.empty_like(W)
            db = torch.empty(W.shape[0], dtype=torch.float32, device=W.device) if ctx.has_bias else None
            ops.linear_backward_params(dy, x, dW, db)
        return dx, dW, db


def hip_linear(x, layer):
    return _LinearFn.apply(x, layer.weight, layer.bias)


class _UpperSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ops = default_ops()
        x = _dense(x)
        S = torch.empty_like(x)
        U = torch.empty_like(x)
        ops.upper_softmax_forward(x, S, U)
        ctx.save_for_backward(S)
        return U

    @staticmethod
    def backward(ctx, gU):
        ops = default_ops()
        (S,) = ctx.saved_tensors
        dl = torch.empty_like(S)
        ops.mask_backward(_dense(gU), S, None, 0.0, 0, dl)
        return dl


class upper_softmax(nn.Module):
    """Upper softmax activation (src/models/Generator.py:6-22): softmax entries >= 1/d snap to 1."""

    def __init__(self):
        super().__init__()

    def forward(self, x):
        return _UpperSoftmaxFn.apply(x)


class _Chain(nn.Module):
    """``self.main = nn.Sequential(Linear...)`` with the reference's state_dict keys; forward runs
    each Linear through the HIP GEMM instead of ATen."""

    def _run(self, x):
        for m in self.main:
            x = hip_linear(x, m) if isinstance(m, nn.Linear) else m(x)
        return x


class Generator_big(_Chain):
    """src/models/Generator.py:58-70: Linear(L,2L) -> (2L,4L) -> (4L,8L) -> (8L,d) -> upper_softmax."""

    def __init__(self, latent_size, img_size):
        super().__init__()
        self.main = nn.Sequential(
            nn.Linear(latent_size, 2 * latent_size),
            nn.Linear(2 * latent_size, 4 * latent_size),
            nn.Linear(4 * latent_size, 8 * latent_size),
            nn.Linear(8 * latent_size, img_size),
            upper_softmax(),
        )

    def forward(self, input):
        return self._run(input)


class Encoder(_Chain):
    """src/models/Detector.py:5-18."""

    def __init__(self, latent_size, img_size):
        super().__init__()
        self.main = nn.Sequential(
            nn.Linear(img_size, 8 * latent_size),
            nn.Linear(8 * latent_size, 4 * latent_size),
            nn.Linear(4 * latent_size, 2 * latent_size),
            nn.Linear(2 * latent_size, latent_size),
        )

    def forward(self, input):
        return self._run(input)


class Decoder(_Chain):
    """src/models/Detector.py:21-34."""

    def __init__(self, latent_size, img_size):
        super().__init__()
        self.main = nn.Sequential(
            nn.Linear(latent_size, 2 * latent_size),
            nn.Linear(2 * latent_size, 4 * latent_size),
            nn.Linear(4 * latent_size, 8 * latent_size),
            nn.Linear(8 * latent_size, img_size),
        )

    def forward(self, input):
        return self._run(input)


class Detector(nn.Module):
    """src/models/Detector.py:37-48: forward(x) -> (enc [n,L], dec [n,d])."""

    def __init__(self, latent_size, img_size, encoder, decoder):
        super().__init__()
        self.encoder = encoder(latent_size, img_size)
        self.decoder = decoder(latent_size, img_size)

    def forward(self, input):
        enc_X = self.encoder(input)
        dec_X = self.decoder(enc_X)
        return enc_X.view(input.size(0), -1), dec_X.view(input.size(0), -1)


class _RBFMatrixFn(torch.autograd.Function):
    """K = RBF(Z) as an N x N matrix (src/models/Mmd_loss_constrained.py:24-26) with autograd to Z: for an upstream gK,
    dZ_i = 2 sum_j W_ij (z_i - z_j) with W = (gK + gK^T) * dK/dL -- the backward product of the MMD (vgan_mmd_backward)."""

    @staticmethod
    def forward(ctx, Z, kernel):
        ops = default_ops()
        N, p = Z.shape
        pp = _round4(p)
        Zp = torch.zeros(N, pp, dtype=torch.float32, device=Z.device)
        Zp[:, :p].copy_(Z)
        sq = torch.empty(N, dtype=torch.float32, device=Z.device)
        ops.row_sqnorm(Zp, sq, pp)
        bw = kernel._device_bandwidth(Zp, sq, N, pp)
        K = torch.empty(N, N, dtype=torch.float32, device=Z.device)
        dK = torch.empty(N, N, dtype=torch.float32, device=Z.device) if ctx.needs_input_grad[0] else None
        ops.rbf_multi_kernel_matrix(Zp, sq, bw, kernel.bandwidth_multipliers.tolist(), K, dK)
        ctx.save_for_backward(Zp, dK)
        ctx.p = p
        return K

    @staticmethod
    def backward(ctx, gK):
        ops = default_ops()
        Zp, dK = ctx.saved_tensors
        N, pp = Zp.shape
        W = ((gK + gK.t()) * dK).contiguous()
        out = torch.empty(N, pp, dtype=torch.float32, device=Zp.device)
        ops.mmd_backward(W, Zp, 0, N, N, pp, None, out)
        return out[:, :ctx.p], None


class RBF(nn.Module):
    """src/models/Mmd_loss_constrained.py:5-26.  Holds the multipliers ``mul_factor ** (arange(n_kernels) - n_kernels // 2)``
    and the bandwidth, which is computed on the first call and frozen.  ``forward(Z)`` returns the N x N kernel matrix like
    the reference's (for callers of the stand-alone module; MMDLossConstrained never materialises it).  The reference's
    defaults (n_kernels=5, mul_factor=2) run the fused one-exp squaring chain; any other setting one exp per kernel."""

    def __init__(self, n_kernels=5, mul_factor=2.0, bandwidth=None):
        super().__init__()
        if not (1 <= int(n_kernels) <= 8):
            raise ValueError(f"RBF: n_kernels must be in 1..8 on the HIP kernels, got {n_kernels}")
        if not float(mul_factor) > 0.0:
            raise ValueError(f"RBF: mul_factor must be positive, got {mul_factor}")
        self.n_kernels, self.mul_factor = int(n_kernels), mul_factor
        self.bandwidth_multipliers = mul_factor ** (torch.arange(n_kernels) - n_kernels // 2)
        self.bandwidth = bandwidth

    def is_default(self):
        return self.n_kernels == 5 and float(self.mul_factor) == 2.0

    def _device_bandwidth(self, Zp, sq, N, pp, n_half=None):
        """The frozen bandwidth as a device scalar [1]; the first call calibrates it from Zp (Mmd_loss_constrained.py:16-22:
        sum of all squared distances / (N^2 - N)).  N must be even here only when n_half is given (the MMD's stacked operand)."""
        ops = default_ops()
        dev = Zp.device
        if self.bandwidth is None:
            # sum over all ordered pairs = 2 * (strict upper triangle); the tile table of an n-row "XX" block does exactly that
            tiles = _tile_cache(ops, N, 0, dev, whole=True)
            partial = torch.empty(tiles.shape[0], 4, dtype=torch.float32, device=dev)
            stats = torch.empty(4, dtype=torch.float64, device=dev)
            bw = torch.empty(1, dtype=torch.float32, device=dev)
            ops.mmd_gram(Zp, sq, N, pp, None, tiles, True, None, 0, partial)
            ops.mmd_reduce(partial, tiles, stats, True)
            stats[3:4].div_(float(N) * N - N)
            bw.copy_(stats[3:4])
            self.bandwidth = bw.view(())
        bw = self.bandwidth
        if not (torch.is_tensor(bw) and bw.is_cuda and bw.dtype == torch.float32):
            bw = torch.as_tensor(float(bw), dtype=torch.float32, device=dev)
        return bw.reshape(1)

    def forward(self, X):
        if X.dim() != 2:
            raise ValueError(f"RBF.forward expects a 2-D tensor [N, p], got {tuple(X.shape)}")
        return _RBFMatrixFn.apply(_dense(X.float()), self)


_TILE_TABLES = {}


def _tile_cache(ops, n, grad_mode, dev, whole=False):
    """Tile tables are a pure function of (n, grad_mode): built and uploaded once per process and device.  whole=True: the
    table of ONE symmetric n x n block (upper triangle, counted twice off the diagonal) -- used to sum all pair distances."""
    key = (int(n), int(grad_mode), str(dev), bool(whole))
    t = _TILE_TABLES.get(key)
    if t is None:
        t = ops.build_tiles(n, grad_mode, device=dev)
        if whole:  # keep the XX tiles of the table only (slot 0): rows/cols in [0, n)
            t = t[(t[:, 4] & 3) == 0].contiguous()
        _TILE_TABLES[key] = t
    return t


class _MMDLossFn(torch.autograd.Function):
    """loss = MMD^2(X, Y) + weight * mean_j(1 - max_i U_ij), fused Gram/kernel-sum tiles on the MFMA."""

    @staticmethod
    def forward(ctx, X, Y, U, weight, kernel):
        ops = default_ops()
        dev = X.device
        n, p = X.shape
        d = U.shape[1]
        pp = _round4(p)
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_mode = 2 if need_x else (1 if need_y else 0)
        Z = torch.zeros(2 * n, pp, dtype=torch.float32, device=dev)
        Z[:n, :p].copy_(X)
        Z[n:, :p].copy_(Y)
        sq = torch.empty(2 * n, dtype=torch.float32, device=dev)
        ops.row_sqnorm(Z, sq, pp)
        tiles = _tile_cache(ops, n, grad_mode, dev)
        partial = torch.empty(tiles.shape[0], 4, dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.float64, device=dev)
        if kernel.bandwidth is None:  # first call calibrates and freezes (Mmd_loss_constrained.py:16-20)
            bw = torch.empty(1, dtype=torch.float32, device=dev)
            ops.mmd_gram(Z, sq, n, pp, None, tiles, True, None, 0, partial)
            ops.mmd_reduce(partial, tiles, stats, True)
            ops.mmd_set_bandwidth(stats, n, bw)
            kernel.bandwidth = bw.view(())
        bw = kernel.bandwidth
        if not (torch.is_tensor(bw) and bw.is_cuda and bw.dtype == torch.float32):
            bw = torch.as_tensor(float(bw), dtype=torch.float32, device=dev)
        bw = bw.reshape(1)
        Wg = wrow0 = None
        if grad_mode == 1:
            Wg, wrow0 = torch.empty(n, 2 * n, dtype=torch.float32, device=dev), n
        elif grad_mode == 2:
            Wg, wrow0 = torch.empty(2 * n, 2 * n, dtype=torch.float32, device=dev), 0
        if kernel.is_default():
            ops.mmd_gram(Z, sq, n, pp, bw, tiles, False, Wg, wrow0 or 0, partial)
        else:
            ops.mmd_gram_general(Z, sq, n, pp, bw, tiles, kernel.bandwidth_multipliers.tolist(), Wg, wrow0 or 0, partial)
        ops.mmd_reduce(partial, tiles, stats, True)
        Uc = _dense(U.detach())
        colpart = torch.empty(ops.colmax_chunks(n) * d, dtype=torch.int64, device=dev)
        colkey = torch.empty(d, dtype=torch.int64, device=dev)
        ops.colmax(Uc, 0, colpart, colkey, False)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ops.mmd_loss(stats, colkey, n, d, float(weight), loss)
        if Wg is not None:
            ctx.save_for_backward(Z, colkey, Wg)
        else:
            ctx.save_for_backward(Z, colkey)
        ctx.wrow0, ctx.dims, ctx.weight, ctx.grad_mode = wrow0, (n, p, pp, d), float(weight), grad_mode
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        ops = default_ops()
        Z, colkey = ctx.saved_tensors[:2]
        n, p, pp, d = ctx.dims
        dX = dY = dU = None
        if ctx.grad_mode:
            Wg = ctx.saved_tensors[2]
            nr = n if ctx.grad_mode == 1 else 2 * n
            out = torch.empty(nr, pp, dtype=torch.float32, device=Z.device)
            ops.mmd_backward(Wg, Z, ctx.wrow0, nr, 2 * n, pp, None, out)
            out = out[:, :p] * gl
            if ctx.grad_mode == 1:
                dY = out
            else:
                dX, dY = out[:n], out[n:]
        if ctx.needs_input_grad[2]:
            rows = 0xFFFFFFFF - (colkey & 0xFFFFFFFF)  # arg-max row per column (lowest row on ties)
            dU = torch.zeros(n, d, dtype=torch.float32, device=Z.device)
            dU[rows, torch.arange(d, device=Z.device)] = -ctx.weight / d
            dU = dU * gl
        return dX, dY, dU, None, None


class _MMDLossUnequalFn(torch.autograd.Function):
    """MMDLossConstrained for X [n_x, p] and Y [n_y, p] with n_x != n_y (and U with any row count), as
    src/models/Mmd_loss_constrained.py:42-50 computes it: block means of K([X; Y]) over n_x^2, n_x n_y and n_y^2 entries.  The
    training step never takes this path (its Y is a function of U * X: equal shapes, fused tile tables); here the N x N kernel
    matrix is materialised by vgan_rbf_multi_kernel_matrix, the block sums are float64 row dots against a row of ones
    (vgan_rows_dot / vgan_sum_f64), and the gradient is the MMD backward product on W = (gK + gK^T) * dK/dL with gK the
    block-constant upstream gradient of the three means."""

    @staticmethod
    def forward(ctx, X, Y, U, weight, kernel):
        ops = default_ops()
        dev = X.device
        nx, p = X.shape
        ny, d = Y.shape[0], U.shape[1]
        N, pp = nx + ny, _round4(p)
        Z = torch.zeros(N, pp, dtype=torch.float32, device=dev)
        Z[:nx, :p].copy_(X)
        Z[nx:, :p].copy_(Y)
        sq = torch.empty(N, dtype=torch.float32, device=dev)
        ops.row_sqnorm(Z, sq, pp)
        bw = kernel._device_bandwidth(Z, sq, N, pp)  # first call: sum of all squared distances of the stacked rows / (N^2 - N)
        Np = _round4(N)
        K = torch.zeros(N, Np, dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dK = torch.zeros(N, Np, dtype=torch.float32, device=dev) if need else None
        ops.rbf_multi_kernel_matrix(Z, sq, bw, kernel.bandwidth_multipliers.tolist(), K, dK)
        ones = torch.ones(1, Np, dtype=torch.float32, device=dev)
        rows = torch.empty(N, dtype=torch.float64, device=dev)
        sums = torch.zeros(3, dtype=torch.float32, device=dev)
        stats = torch.zeros(4, dtype=torch.float64, device=dev)
        for slot, (r0, r1, c0, c1) in enumerate(((0, nx, 0, nx), (0, nx, nx, N), (nx, N, nx, N))):  # XX, XY, YY
            ops.rows_dot(K[r0:r1, c0:c1], ones[:, :c1 - c0], rows, broadcast_b=True)
            ops.sum_f64(rows, r1 - r0, 1.0 / (float(r1 - r0) * float(c1 - c0)), sums[slot:slot + 1])
        stats[:3].copy_(sums)  # the three block MEANS; vgan_mmd_loss then forms xx - 2 xy + yy (its n = 1) + the penalty
        Uc = _dense(U.detach().float())
        colpart = torch.empty(ops.colmax_chunks(Uc.shape[0]) * d, dtype=torch.int64, device=dev)
        colkey = torch.empty(d, dtype=torch.int64, device=dev)
        ops.colmax(Uc, 0, colpart, colkey, False)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ops.mmd_loss(stats, colkey, 1, d, float(weight), loss)
        ctx.save_for_backward(Z, colkey, dK) if need else ctx.save_for_backward(Z, colkey)
        ctx.dims, ctx.weight, ctx.nu = (nx, ny, p, pp, d), float(weight), Uc.shape[0]
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        ops = default_ops()
        Z, colkey = ctx.saved_tensors[:2]
        nx, ny, p, pp, d = ctx.dims
        N = nx + ny
        dX = dY = dU = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # W = dK/dL scaled by (gK + gK^T): 2 / n_x^2 | -2 / (n_x n_y) | 2 / n_y^2 per block, formed in a buffer of its own:
            # dK is a saved tensor, and a retained graph may be differentiated again
            dK = ctx.saved_tensors[2]
            W = torch.zeros_like(dK)
            torch.mul(dK[:nx, :nx], 2.0 / (float(nx) * nx), out=W[:nx, :nx])
            torch.mul(dK[:nx, nx:N], -2.0 / (float(nx) * ny), out=W[:nx, nx:N])
            torch.mul(dK[nx:, :nx], -2.0 / (float(nx) * ny), out=W[nx:, :nx])
            torch.mul(dK[nx:, nx:N], 2.0 / (float(ny) * ny), out=W[nx:, nx:N])
            out = torch.empty(N, pp, dtype=torch.float32, device=Z.device)
            ops.mmd_backward(W, Z, 0, N, N, pp, None, out)
            out = out[:, :p] * gl
            dX, dY = out[:nx], out[nx:]
        if ctx.needs_input_grad[2]:
            rows = 0xFFFFFFFF - (colkey & 0xFFFFFFFF)
            dU = torch.zeros(ctx.nu, d, dtype=torch.float32, device=Z.device)
            dU[rows, torch.arange(d, device=Z.device)] = -ctx.weight / d
            dU = dU * gl
        return dX, dY, dU, None, None


class MMDLossConstrained(nn.Module):
    """src/models/Mmd_loss_constrained.py:29-50.  As in the reference, the default ``kernel=RBF()`` is
    evaluated once at class-definition time: every instance created without an explicit kernel
    shares ONE RBF and therefore one frozen bandwidth per process (reference quirk, kept)."""

    def __init__(self, weight, kernel=RBF()):
        super().__init__()
        self.kernel = kernel
        self.weight = weight

    def forward(self, X, Y, U):
        if X.dim() != 2 or Y.dim() != 2 or X.shape[1] != Y.shape[1]:
            raise ValueError(f"MMDLossConstrained: X and Y must be 2-D with the same number of columns, got {tuple(X.shape)} and "
                             f"{tuple(Y.shape)}")
        if U.dim() != 2:
            raise ValueError(f"MMDLossConstrained: U must be 2-D [rows, d], got {tuple(U.shape)}")
        # the reference takes block means over arbitrary row counts of X and Y (Mmd_loss_constrained.py:46-49); every caller in
        # the reference passes Y = f(U * X), i.e. equal shapes: that is the fused tile path.  Anything else (n_x != n_y, or a U
        # with another row count) takes the general path on the materialised kernel matrix.
        fn = _MMDLossFn if (Y.shape == X.shape and U.shape[0] == X.shape[0]) else _MMDLossUnequalFn
        out = fn.apply(_dense(X.float()), _dense(Y.float()), U, self.weight, self.kernel)
        self.bandwidth = self.kernel.bandwidth
        self.bandwidth_multipliers = self.kernel.bandwidth_multipliers
        return out

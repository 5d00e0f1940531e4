"""Kernel provider: the one place that turns torch tensors into C-ABI calls (include/vgan_hip.h).

``HipOps`` is the product's only provider.  Every method launches asynchronously on torch's
current HIP stream (so calls can be captured into a HIP graph) and writes into caller-owned
tensors.  A provider with the same method set over CPU tensors exists only under ``tests/`` to
exercise the host logic (fit loop, sharding, collectives) without a GPU.
"""
import ctypes

import torch

from . import lib as _lib

_f32 = torch.float32


def _round4(v):
    return (int(v) + 3) // 4 * 4


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _mat(t, name):
    if not (t.is_cuda and t.dtype == _f32 and t.dim() == 2 and t.stride(1) == 1):
        raise ValueError(f"{name}: need a float32 HIP matrix with unit inner stride, got "
                         f"{t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    return t


def _vec(t, name, dtype=_f32):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous {dtype} HIP tensor, got {t.dtype} on {t.device}")
    return t


class HipOps:
    """libvgan_hip.so on the current device/stream.  Raises if the library or a GPU is missing."""

    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.VganHipError("vgan_amd needs a HIP device (torch.cuda.is_available() is False); "
                                    "there is no CPU fallback")

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- host helpers -----------------------------------------------------------------------
    def build_tiles(self, n, grad_mode, rank=0, world=1, device=None, tile=64, split_xx=False, split=None):
        """split_xx (= split "xx_last"): the table is returned as [XY and YY tiles ... | XX tiles ...] (each part in XCD order)
        together with the length of the first part, for callers that launch the sum-only XX tiles separately; split "yy_last":
        [XY and XX tiles ... | YY tiles ...] (the sharded data-parallel front: the first part needs no other rank's rows)."""
        flat, cnt = _lib.build_tiles(n, grad_mode, rank, world, tile)
        table = torch.tensor(flat, dtype=torch.int32).view(cnt, 8)
        if split_xx or split:
            first, second = _lib.split_tiles(table, tile, yy_last=(split == "yy_last"))
            return torch.cat([first, second]).to(device or "cuda"), first.shape[0]
        return table.to(device or "cuda")

    def colmax_chunks(self, n):
        return self.lib.vgan_colmax_chunks(n)

    # ---- Linear ------------------------------------------------------------------------------
    def linear_forward(self, x, W, b, y, x_nslabs=1, x_slab_stride=0):
        """x_nslabs > 1: `x` is slab 0 of unreduced split-K slabs `x_slab_stride` elements apart (summed while staged)."""
        _mat(x, "x"), _mat(W, "W"), _mat(y, "y")
        n, kin = x.shape
        out = W.shape[0]
        assert W.shape[1] == kin and y.shape == (n, out)
        _lib.check(self.lib.vgan_linear_forward(_ptr(x), x.stride(0), int(x_nslabs), int(x_slab_stride), _ptr(W), W.stride(0),
                                                _ptr(b), _ptr(y), y.stride(0), n, kin, out, self._stream()), "vgan_linear_forward")

    def linear_forward_path(self, x, W, b, y, x_nslabs=1, x_slab_stride=0):
        """The kernel linear_forward launches for exactly these arguments (lib.LINEAR_FORWARD_PATHS; host-side query)."""
        n, kin = x.shape
        return _lib.path_name(_lib.LINEAR_FORWARD_PATHS, self.lib.vgan_linear_forward_path(
            _ptr(x), x.stride(0), int(x_nslabs), int(x_slab_stride), _ptr(W), W.stride(0), _ptr(b), _ptr(y), y.stride(0), n, kin,
            W.shape[0]), "vgan_linear_forward_path")

    def linear_backward_input(self, dy, W, dx):
        _mat(dy, "dy"), _mat(W, "W"), _mat(dx, "dx")
        n, out = dy.shape
        kin = W.shape[1]
        assert W.shape[0] == out and dx.shape == (n, kin)
        _lib.check(self.lib.vgan_linear_backward_input(_ptr(dy), dy.stride(0), _ptr(W), W.stride(0), _ptr(dx), dx.stride(0),
                                                       n, kin, out, self._stream()), "vgan_linear_backward_input")

    def linear_backward_input_path(self, dy, W, dx):
        """The kernel linear_backward_input launches for exactly these arguments (lib.LINEAR_BACKWARD_INPUT_PATHS)."""
        n, out = dy.shape
        return _lib.path_name(_lib.LINEAR_BACKWARD_INPUT_PATHS, self.lib.vgan_linear_backward_input_path(
            _ptr(dy), dy.stride(0), _ptr(W), W.stride(0), _ptr(dx), dx.stride(0), n, W.shape[1], out), "vgan_linear_backward_input_path")

    def linear_backward_params(self, dy, x, dW, db, splits=1, slab_stride=0, x_nslabs=1, x_slab_stride=0):
        """splits > 1: dW/db are slab 0 of `splits` slabs `slab_stride` elements apart (partial sums).
        x_nslabs > 1: `x` itself is slab 0 of unreduced slabs (summed while staged)."""
        _mat(dy, "dy"), _mat(x, "x"), _mat(dW, "dW")
        n, out = dy.shape
        kin = x.shape[1]
        assert x.shape[0] == n and dW.shape == (out, kin)
        _lib.check(self.lib.vgan_linear_backward_params(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), int(x_nslabs), int(x_slab_stride),
                                                        _ptr(dW), dW.stride(0), _ptr(db), n, kin, out, int(splits), int(slab_stride),
                                                        self._stream()), "vgan_linear_backward_params")

    def linear_backward_params_path(self, dy, x, dW, db, splits=1, slab_stride=0, x_nslabs=1, x_slab_stride=0):
        """The kernel linear_backward_params launches for exactly these arguments (lib.LINEAR_BACKWARD_PARAMS_PATHS)."""
        n, out = dy.shape
        return _lib.path_name(_lib.LINEAR_BACKWARD_PARAMS_PATHS, self.lib.vgan_linear_backward_params_path(
            _ptr(dy), dy.stride(0), _ptr(x), x.stride(0), int(x_nslabs), int(x_slab_stride), _ptr(dW), dW.stride(0), _ptr(db), n,
            x.shape[1], out, int(splits), int(slab_stride)), "vgan_linear_backward_params_path")

    def linear_backward_params_ksplit_ws_bytes(self, kin, out, parts):
        return int(self.lib.vgan_linear_backward_params_ksplit_ws_bytes(int(kin), int(out), int(parts)))

    def ksplit_workspace(self, nbytes, device=None):
        """A zeroed workspace for the in-launch K split (tickets first, then slabs): allocate once, never share between
        launches that may overlap."""
        return torch.zeros(max(int(nbytes), 16) // 4 + 4, dtype=torch.int32, device=device or "cuda")

    def linear_backward_params_ksplit(self, dy, x, dW, parts, ws):
        """linear_backward_params (no bias, no slabs) with every output tile's contraction cut over `parts` workgroups and
        combined inside the launch (deterministic); `ws` = ksplit_workspace(linear_backward_params_ksplit_ws_bytes(...)) or None
        for parts == 1, which is linear_backward_params itself."""
        _mat(dy, "dy"), _mat(x, "x"), _mat(dW, "dW")
        n, out = dy.shape
        kin = x.shape[1]
        assert x.shape[0] == n and dW.shape == (out, kin)
        _lib.check(self.lib.vgan_linear_backward_params_ksplit(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dW), dW.stride(0), n, kin, out,
                                                               int(parts), _ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(),
                                                               self._stream()), "vgan_linear_backward_params_ksplit")

    def linear_backward_params_xx_supported(self, n, kin, out):
        return bool(self.lib.vgan_linear_backward_params_xx_supported(int(n), int(kin), int(out)))

    def linear_backward_params_xx(self, dy, x, dW, xx):
        """linear_backward_params (no bias, no slabs) with an xx_job() riding in the launch (the step's M_4 product)."""
        _mat(dy, "dy"), _mat(x, "x"), _mat(dW, "dW")
        n, out = dy.shape
        kin = x.shape[1]
        assert x.shape[0] == n and dW.shape == (out, kin)
        _lib.check(self.lib.vgan_linear_backward_params_xx(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dW), dW.stride(0), n, kin, out,
                                                           ctypes.byref(xx), self._stream()), "vgan_linear_backward_params_xx")

    def reduce_slabs(self, src, slab_stride, nslabs, dst):
        _vec(dst, "dst")
        _lib.check(self.lib.vgan_reduce_slabs(_ptr(src), int(slab_stride), int(nslabs), _ptr(dst), dst.numel(), self._stream()),
                   "vgan_reduce_slabs")

    # ---- upper_softmax / projection ------------------------------------------------------------
    def col_mean(self, data, out):
        """out[d] = per-feature mean of data [rows, d]: the centre the step engine subtracts from the MMD operand."""
        _mat(data, "data"), _vec(out, "out")
        rows, d = data.shape
        assert out.numel() >= d
        _lib.check(self.lib.vgan_col_mean(_ptr(data), data.stride(0), rows, d, _ptr(out), self._stream()), "vgan_col_mean")

    @staticmethod
    def logits_chain(za, At4):
        """The collapsed generator as a job for mask_project_forward(_bf3) (`chain=`): logits = za . At4^T are formed inside that
        launch.  za [n, e0] = [z | 1 | 0-pad], At4 [d, e0].  Raw pointers: the tensors must outlive every launch using the job."""
        _mat(za, "za"), _mat(At4, "At4")
        assert za.shape[1] == At4.shape[1]
        return _lib.LogitsChain(_ptr(za), _ptr(At4), za.stride(0), At4.stride(0), za.shape[1], 0)

    @staticmethod
    def chain_fusable(n, d, *lds):
        return d % 4 == 0 and d <= 1024 and all(int(v) % 4 == 0 for v in lds)

    def mask_project_forward(self, logits, data, rows, S, U, Zx, Zy, sqx, sqy, row_cursor=None, row_batches=1, row_stride=0,
                             row_offset=0, center=None, norm_split=False, chain=None):
        """center [d]: subtracted from every row written to Zx / Zy; norm_split: sqx / sqy are the norms of the bf16 hi + lo
        split of those rows (what mmd_gram_bf3 needs); chain: a logits_chain() -- `logits` is then not read (may be None)."""
        _mat(data, "data"), _mat(Zy, "Zy"), _mat(S, "S")
        n, d = S.shape
        if logits is not None:
            _mat(logits, "logits")
            assert tuple(logits.shape) == (n, d)
        assert S.is_contiguous() and S.shape == (n, d) and (U is None or (U.is_contiguous() and U.shape == (n, d)))
        assert Zx is None or Zx.stride(0) == Zy.stride(0)
        if rows is not None:
            _vec(rows, "rows", torch.int32)
        _lib.check(self.lib.vgan_mask_project_forward(_ptr(logits), logits.stride(0) if logits is not None else 0, _ptr(data), data.stride(0), _ptr(rows),
                                                      _ptr(row_cursor), int(row_batches), int(row_stride), int(row_offset), _ptr(S), _ptr(U), _ptr(Zx), _ptr(Zy), Zy.stride(0), _ptr(sqx), _ptr(sqy),
                                                      n, d, _ptr(center), int(bool(norm_split)),
                                                      ctypes.byref(chain) if chain is not None else None, self._stream()), "vgan_mask_project_forward")

    # this provider has the launches of the bf16x3 step without an fp32 operand copy: mask_project_forward_bf3(write_z=, xrow=)
    # and mmd_backward_bf3_rm_rebuild
    bf3_rebuild = True
    chain_ksplit = True  # linear_backward_params_ksplit and gemm_grouped(kparts=...)

    def xx_job(self, Dh, Dl, dsq, tiles, bw, partial):
        """The X-X Gram tiles as a job for mask_project_forward_bf3 (`xx=`): Dh, Dl, dsq = split images / norms of the whole
        (centred) data set, tiles / partial = the X-X part of the tile table and of the partial buffer.  Raw pointers: the
        tensors must outlive every launch (and graph replay) that uses the job."""
        assert tiles.is_contiguous() and partial.is_contiguous() and Dh.stride(0) == Dl.stride(0)
        return _lib.XXJob(_ptr(Dh), _ptr(Dl), _ptr(dsq), _ptr(tiles), _ptr(bw), _ptr(partial), Dh.stride(0), tiles.shape[0])

    def bwd_rebuild(self, data, xrow, S, center):
        """What mmd_backward_bf3_rm_rebuild forms its epilogue operands from (raw pointers: the tensors must outlive the job)."""
        _mat(data, "data"), _mat(S, "S")
        assert xrow.dtype == torch.int32 and xrow.is_contiguous() and center.is_contiguous()
        return _lib.BwdRebuild(_ptr(data), _ptr(xrow), _ptr(S), _ptr(center), data.stride(0), S.stride(0))

    def mask_project_forward_bf3(self, logits, data, rows, S, Z, sq, Zh, Zl, ZTh, ZTl, row_cursor=None, row_batches=1, row_stride=0,
                                 center=None, write_x=True, xx=None, chain=None, write_z=True, xrow=None):
        """mask_project_forward + mmd_bf3_prepare in one launch (shape contract in include/vgan_hip.h; see bf3_fusable).
        write_z=False: the fp32 operand Z is not written; xrow: int32 [n], receives the data-set row of every batch row."""
        _mat(data, "data"), _mat(Z, "Z"), _mat(S, "S")
        n, d = S.shape
        if logits is not None:
            _mat(logits, "logits")
        if not write_z or xrow is not None:
            _lib.check(self.lib.vgan_mask_project_forward_bf3_ex(_ptr(logits), logits.stride(0) if logits is not None else 0, _ptr(data),
                                                                 data.stride(0), _ptr(rows), _ptr(row_cursor), int(row_batches),
                                                                 int(row_stride), _ptr(S), _ptr(Z), Z.stride(0), _ptr(sq), _ptr(Zh), _ptr(Zl),
                                                                 Zh.stride(0), _ptr(ZTh), _ptr(ZTl), ZTh.stride(0) if ZTh is not None else 0,
                                                                 n, d, _ptr(center), int(bool(write_x)),
                                                                 ctypes.byref(xx) if xx is not None else None,
                                                                 ctypes.byref(chain) if chain is not None else None, int(bool(write_z)),
                                                                 _ptr(xrow), self._stream()), "vgan_mask_project_forward_bf3_ex")
            return
        _lib.check(self.lib.vgan_mask_project_forward_bf3(_ptr(logits), logits.stride(0) if logits is not None else 0, _ptr(data), data.stride(0), _ptr(rows),
                                                          _ptr(row_cursor), int(row_batches), int(row_stride), _ptr(S), _ptr(Z), Z.stride(0),
                                                          _ptr(sq), _ptr(Zh), _ptr(Zl), Zh.stride(0), _ptr(ZTh), _ptr(ZTl),
                                                          ZTh.stride(0) if ZTh is not None else 0,
                                                          n, d, _ptr(center), int(bool(write_x)),
                                                          ctypes.byref(xx) if xx is not None else None,
                                                          ctypes.byref(chain) if chain is not None else None, self._stream()),
                   "vgan_mask_project_forward_bf3")

    @staticmethod
    def bf3_fusable(n, d, *lds):
        return d % 4 == 0 and d <= 1024 and n % 8 == 0 and all(int(v) % 4 == 0 for v in lds)

    def gather_rows(self, data, rows, out, sq, row_cursor=None, row_batches=1, row_stride=0, row_offset=0):
        _mat(data, "data"), _mat(out, "out")
        n, d = out.shape[0], data.shape[1]
        _lib.check(self.lib.vgan_gather_rows(_ptr(data), data.stride(0), _ptr(rows), _ptr(row_cursor), int(row_batches),
                                             int(row_stride), int(row_offset), _ptr(out), out.stride(0), _ptr(sq), n, d,
                                             self._stream()), "vgan_gather_rows")

    def gather_rows_split(self, data, rows, center, out, sq, norm_split=False, Zh=None, Zl=None, row_cursor=None, row_batches=1,
                          row_stride=0, row_offset=0, n=None):
        """X half of the centred MMD operand for the batch the cursor points at: out / sq / split images (each optional)."""
        _mat(data, "data")
        d = data.shape[1]
        n = int(n if n is not None else (out.shape[0] if out is not None else sq.numel()))
        _lib.check(self.lib.vgan_gather_rows_split(_ptr(data), data.stride(0), _ptr(rows), _ptr(row_cursor), int(row_batches),
                                                   int(row_stride), int(row_offset), _ptr(center), _ptr(out),
                                                   out.stride(0) if out is not None else 0, _ptr(sq), int(bool(norm_split)), _ptr(Zh),
                                                   _ptr(Zl), Zh.stride(0) if Zh is not None else 0, n, d, self._stream()),
                   "vgan_gather_rows_split")

    def upper_softmax_forward(self, logits, S, U):
        _mat(logits, "logits")
        n, d = logits.shape
        assert S.is_contiguous() and (U is None or U.is_contiguous())
        _lib.check(self.lib.vgan_upper_softmax_forward(_ptr(logits), logits.stride(0), _ptr(S), _ptr(U), n, d, self._stream()),
                   "vgan_upper_softmax_forward")

    def mask_backward(self, gU, S, colkey, pen_weight, row_offset, dlogits, nslabs=1, slab_stride=0):
        _mat(gU, "gU"), _mat(S, "S"), _mat(dlogits, "dlogits")
        n, d = S.shape
        _lib.check(self.lib.vgan_mask_backward(_ptr(gU), gU.stride(0), int(nslabs), int(slab_stride), _ptr(S), S.stride(0),
                                               _ptr(colkey), float(pen_weight),
                                               int(row_offset), _ptr(dlogits), dlogits.stride(0), n, d, self._stream()),
                   "vgan_mask_backward")

    def colmax(self, S, row_offset, part, colkey, from_softmax=True):
        _mat(S, "S")
        n, d = S.shape
        assert part.dtype == torch.int64 and colkey.dtype == torch.int64 and part.numel() >= self.colmax_chunks(n) * d
        _lib.check(self.lib.vgan_colmax(_ptr(S), S.stride(0), int(bool(from_softmax)), int(row_offset), _ptr(part), _ptr(colkey), n, d, self._stream()),
                   "vgan_colmax")

    def colmax_partial(self, S, row_offset, part, from_softmax=True):
        _mat(S, "S")
        n, d = S.shape
        assert part.dtype == torch.int64 and part.numel() >= self.colmax_chunks(n) * d
        _lib.check(self.lib.vgan_colmax_partial(_ptr(S), S.stride(0), int(bool(from_softmax)), int(row_offset), _ptr(part), n, d,
                                                self._stream()), "vgan_colmax_partial")

    def mmd_finalize(self, partial, tiles, colpart, chunks, colkey, n, d, weight, stats, loss, loss_accum=None, accum_scale=1.0,
                     step_counter=None):
        _lib.check(self.lib.vgan_mmd_finalize(_ptr(partial), _ptr(tiles), tiles.shape[0], _ptr(colpart), int(chunks), _ptr(colkey),
                                              int(n), int(d), float(weight), _ptr(stats), _ptr(loss), _ptr(loss_accum),
                                              float(accum_scale), _ptr(step_counter), self._stream()), "vgan_mmd_finalize")

    def finalize_job(self, partial, tiles, colpart, chunks, colkey, n, d, weight, stats, loss, loss_accum=None, accum_scale=1.0,
                     step_counter=None, mode=0, ntiles_main=0):
        """The arguments of mmd_finalize as a job for mmd_backward / mmd_backward_bf3 (`finalize=`) or gemm_grouped (`fold=`).
        mode 1 / 2: the two halves of a split tail (include/vgan_hip.h: the X-X block sum arrives later in the step).  The job
        holds raw device pointers: the tensors must outlive every launch (and graph replay) that uses it."""
        return _lib.FinalizeJob(_ptr(partial), _ptr(tiles), _ptr(colpart), _ptr(colkey), _ptr(stats), _ptr(loss), _ptr(loss_accum),
                                _ptr(step_counter), tiles.shape[0], int(chunks), int(n), int(d), float(weight), float(accum_scale),
                                int(mode), int(ntiles_main))

    def mask_from_softmax(self, S, U):
        _mat(S, "S"), _mat(U, "U")
        n, d = S.shape
        _lib.check(self.lib.vgan_mask_from_softmax(_ptr(S), S.stride(0), _ptr(U), U.stride(0), n, d, self._stream()),
                   "vgan_mask_from_softmax")

    # ---- MMD -------------------------------------------------------------------------------------
    def row_sqnorm(self, Z, sq, p):
        _mat(Z, "Z")
        _lib.check(self.lib.vgan_row_sqnorm(_ptr(Z), Z.stride(0), _ptr(sq), Z.shape[0], int(p), self._stream()), "vgan_row_sqnorm")

    def mmd_gram(self, Z, sq, n, p, bw, tiles, calibrate, Wg, wrow0, partial):
        _mat(Z, "Z")
        assert (calibrate or Z.shape[0] >= 2 * n) and tiles.dtype == torch.int32 and tiles.is_contiguous()  # (calibration: the table bounds the rows)
        ntiles = tiles.shape[0]
        assert partial.numel() >= 4 * ntiles
        ldw = Wg.stride(0) if Wg is not None else 0
        _lib.check(self.lib.vgan_mmd_gram(_ptr(Z), Z.stride(0), _ptr(sq), int(n), int(p), _ptr(bw), _ptr(tiles), ntiles,
                                          int(bool(calibrate)), _ptr(Wg), ldw, int(wrow0), _ptr(partial), self._stream()),
                   "vgan_mmd_gram")

    @staticmethod
    def _mults(multipliers):
        vals = [float(v) for v in multipliers]
        return (ctypes.c_float * len(vals))(*vals), len(vals)

    def mmd_gram_general(self, Z, sq, n, p, bw, tiles, multipliers, Wg, wrow0, partial):
        """mmd_gram (no calibration) for RBF(n_kernels, mul_factor) other than the reference's defaults: `multipliers` is the
        host list mul_factor ** (k - n_kernels // 2)."""
        _mat(Z, "Z")
        ntiles = tiles.shape[0]
        assert partial.numel() >= 4 * ntiles
        arr, nk = self._mults(multipliers)
        ldw = Wg.stride(0) if Wg is not None else 0
        _lib.check(self.lib.vgan_mmd_gram_general(_ptr(Z), Z.stride(0), _ptr(sq), int(n), int(p), _ptr(bw), _ptr(tiles), ntiles, arr, nk,
                                                  _ptr(Wg), ldw, int(wrow0), _ptr(partial), self._stream()), "vgan_mmd_gram_general")

    def rbf_multi_kernel_matrix(self, Z, sq, bw, multipliers, K, dK=None):
        """RBF.forward: K [m, m] = sum_k exp(-|z_i - z_j|^2 / (bw * multipliers[k])); dK (optional) = dK/dL."""
        _mat(Z, "Z"), _mat(K, "K")
        m, p = Z.shape
        arr, nk = self._mults(multipliers)
        _lib.check(self.lib.vgan_rbf_multi_kernel_matrix(_ptr(Z), Z.stride(0), m, p, _ptr(sq), _ptr(bw), arr, nk, _ptr(K), K.stride(0),
                                                         _ptr(dK), dK.stride(0) if dK is not None else 0, self._stream()),
                   "vgan_rbf_multi_kernel_matrix")

    def mmd_gram_colmax(self, Z, sq, n, p, bw, tiles, Wg, wrow0, partial, S, row_offset, colpart, from_softmax=True):
        """mmd_gram (no calibration) + colmax_partial(S) in one launch."""
        _mat(Z, "Z"), _mat(S, "S")
        ntiles = tiles.shape[0]
        nrows, d = S.shape
        assert partial.numel() >= 4 * ntiles and colpart.dtype == torch.int64 and colpart.numel() >= self.colmax_chunks(nrows) * d
        ldw = Wg.stride(0) if Wg is not None else 0
        _lib.check(self.lib.vgan_mmd_gram_colmax(_ptr(Z), Z.stride(0), _ptr(sq), int(n), int(p), _ptr(bw), _ptr(tiles), ntiles,
                                                 _ptr(Wg), ldw, int(wrow0), _ptr(partial), _ptr(S), S.stride(0),
                                                 int(bool(from_softmax)), int(row_offset), _ptr(colpart), nrows, d, self._stream()),
                   "vgan_mmd_gram_colmax")

    def mmd_reduce(self, partial, tiles, stats, zero_first=True):
        assert stats.dtype == torch.float64 and stats.numel() >= 4
        _lib.check(self.lib.vgan_mmd_reduce(_ptr(partial), _ptr(tiles), tiles.shape[0], _ptr(stats), int(bool(zero_first)),
                                            self._stream()), "vgan_mmd_reduce")

    def mmd_set_bandwidth(self, stats, n, bw):
        _lib.check(self.lib.vgan_mmd_set_bandwidth(_ptr(stats), int(n), _ptr(bw), self._stream()), "vgan_mmd_set_bandwidth")

    def mmd_loss(self, stats, colkey, n, d, weight, loss, loss_accum=None, accum_scale=1.0, step_counter=None):
        _lib.check(self.lib.vgan_mmd_loss(_ptr(stats), _ptr(colkey), int(n), int(d), float(weight), _ptr(loss), _ptr(loss_accum),
                                          float(accum_scale), _ptr(step_counter), self._stream()), "vgan_mmd_loss")

    def mmd_backward(self, Wg, Z, wrow0, nr, ncols, p, mul, out, splits=1, slab_stride=0, finalize=None, mul_shift=None):
        """splits > 1: `out` is slab 0 of `splits` partial slabs `slab_stride` elements apart.  finalize: a finalize_job()
        that one extra workgroup of the launch executes.  mul_shift [p]: added to `mul` (which is stored centred)."""
        _mat(Wg, "Wg"), _mat(Z, "Z"), _mat(out, "out")
        ldmul = mul.stride(0) if mul is not None else 0
        _lib.check(self.lib.vgan_mmd_backward(_ptr(Wg), Wg.stride(0), _ptr(Z), Z.stride(0), int(wrow0), int(nr), int(ncols), int(p),
                                              _ptr(mul), ldmul, _ptr(mul_shift), _ptr(out), out.stride(0), int(splits), int(slab_stride),
                                              ctypes.byref(finalize) if finalize is not None else None, self._stream()),
                   "vgan_mmd_backward")

    # ---- split-bf16 MMD (opt-in precision mode) ------------------------------------------------------
    def mmd_bf3_prepare(self, Z, rows, p, Zh, Zl, ZTh=None, ZTl=None):
        _mat(Z, "Z")
        for t in (Zh, Zl, ZTh, ZTl):
            assert t is None or (t.dtype == torch.int16 and t.is_cuda and t.stride(1) == 1)
        kn = ZTh.stride(0) if ZTh is not None else 0
        _lib.check(self.lib.vgan_mmd_bf3_prepare(_ptr(Z), Z.stride(0), int(rows), int(p), _ptr(Zh), _ptr(Zl), Zh.stride(0),
                                                 _ptr(ZTh), _ptr(ZTl), kn, self._stream()), "vgan_mmd_bf3_prepare")

    def gram_tail_workspace(self, device):
        """Workspace a tile-256 mmd_gram_bf3 launch splits its last round in (include/vgan_hip.h: tail_ws); zeroed once here."""
        return torch.zeros(int(self.lib.vgan_mmd_gram_bf3_tail_ws_bytes()) // 4, dtype=torch.int32, device=device)

    def mmd_gram_bf3(self, Zh, Zl, sq, n, bw, tiles, Wh, Wl, wrow0, partial, S=None, row_offset=0, colpart=None, from_softmax=True,
                     tile=64, tail_ws=None, rs_part=None):
        ntiles = tiles.shape[0]
        nrows, d = (S.shape if S is not None else (0, 0))
        ldw = Wh.stride(0) if Wh is not None else 0
        _lib.check(self.lib.vgan_mmd_gram_bf3(_ptr(Zh), _ptr(Zl), Zh.stride(0), _ptr(sq), int(n), _ptr(bw), _ptr(tiles), ntiles,
                                              int(tile), _ptr(Wh), _ptr(Wl), ldw, int(wrow0), _ptr(partial), _ptr(S),
                                              S.stride(0) if S is not None else 0, int(bool(from_softmax)), int(row_offset),
                                              _ptr(colpart), nrows, d, _ptr(tail_ws), tail_ws.numel() * 4 if tail_ws is not None else 0,
                                              _ptr(rs_part), rs_part.stride(0) if rs_part is not None else 0, self._stream()),
                   "vgan_mmd_gram_bf3")

    def mmd_backward_bf3(self, Wh, Wl, ZTh, ZTl, Z, wrow0, nr, p, mul, out, splits=1, slab_stride=0, finalize=None, mul_shift=None,
                         tile=0):
        """out = 2 (rowsum(W) z - W . Z) (mul + mul_shift) on the TRANSPOSED split images ZTh, ZTl [kp, kn].  tile: 0 = the library's
        rule (mmd_backward_bf3_tile), or 64 / 128 / 256 to force one.  The 256 x 128 tiles read the row-major operand only: on the
        transposed images a rule or a request of 256 runs the 128-wide kernel instead (same bits as tile=128)."""
        _mat(Z, "Z"), _mat(out, "out")
        ldmul = mul.stride(0) if mul is not None else 0
        _lib.check(self.lib.vgan_mmd_backward_bf3(_ptr(Wh), _ptr(Wl), Wh.stride(0), _ptr(ZTh), _ptr(ZTl), ZTh.stride(0),
                                                  ZTh.shape[0], _ptr(Z), Z.stride(0), int(wrow0), int(nr), int(p), _ptr(mul), ldmul,
                                                  _ptr(mul_shift), _ptr(out), out.stride(0), int(splits), int(slab_stride), int(tile),
                                                  ctypes.byref(finalize) if finalize is not None else None, self._stream()),
                   "vgan_mmd_backward_bf3")

    def mmd_backward_bf3_rm(self, Wh, Wl, Zh, Zl, zrows, Z, wrow0, nr, p, mul, out, splits=1, slab_stride=0, finalize=None, mul_shift=None,
                            tile=0, xx=None, rs_part=None):
        """mmd_backward_bf3 on the ROW-MAJOR split images Zh, Zl [>= zrows, kp] (no transposed copies of Z).  xx: an xx_job() whose
        X-X Gram tiles ride in the launch as surplus workgroups (64-wide tiles only).  rs_part: the per-slot row sums of W a
        tile-256 mmd_gram_bf3 launch left (include/vgan_hip.h); read by the 256 x 128 tiles only, and only when every K slab is a
        whole number of 128-column slots.  tile: 0 = the rule of mmd_backward_bf3_tile, or 64 / 128 / 256 to force one."""
        _mat(Z, "Z"), _mat(out, "out")
        ldmul = mul.stride(0) if mul is not None else 0
        kn = (int(zrows) + 63) // 64 * 64
        assert Wh.stride(0) >= kn and Zh.shape[0] >= zrows
        if xx is not None:
            assert tile in (0, 64)
            _lib.check(self.lib.vgan_mmd_backward_bf3_rm_xx(_ptr(Wh), _ptr(Wl), Wh.stride(0), kn, _ptr(Zh), _ptr(Zl), Zh.stride(0), int(zrows),
                                                            _ptr(Z), Z.stride(0), int(wrow0), int(nr), int(p), _ptr(mul), ldmul, _ptr(mul_shift),
                                                            _ptr(out), out.stride(0), int(splits), int(slab_stride),
                                                            ctypes.byref(finalize) if finalize is not None else None, ctypes.byref(xx),
                                                            self._stream()), "vgan_mmd_backward_bf3_rm_xx")
            return
        _lib.check(self.lib.vgan_mmd_backward_bf3_rm(_ptr(Wh), _ptr(Wl), Wh.stride(0), kn, _ptr(Zh), _ptr(Zl), Zh.stride(0), int(zrows),
                                                     _ptr(Z), Z.stride(0), int(wrow0), int(nr), int(p), _ptr(mul), ldmul, _ptr(mul_shift),
                                                     _ptr(out), out.stride(0), int(splits), int(slab_stride), int(tile),
                                                     ctypes.byref(finalize) if finalize is not None else None, _ptr(rs_part),
                                                     rs_part.stride(0) if rs_part is not None else 0, self._stream()),
                   "vgan_mmd_backward_bf3_rm")

    def mmd_backward_bf3_rm_rebuild(self, Wh, Wl, Zh, Zl, zrows, nr, p, rebuild, out, splits=1, slab_stride=0, finalize=None, xx=None):
        """mmd_backward_bf3_rm on 64-wide tiles with the epilogue operands rebuilt from `rebuild` (bwd_rebuild()) instead of read from
        an fp32 Z and its X half: the same bits, without that copy (include/vgan_hip.h)."""
        _mat(out, "out")
        kn = (int(zrows) + 63) // 64 * 64
        assert Wh.stride(0) >= kn and Zh.shape[0] >= zrows
        _lib.check(self.lib.vgan_mmd_backward_bf3_rm_rebuild(_ptr(Wh), _ptr(Wl), Wh.stride(0), kn, _ptr(Zh), _ptr(Zl), Zh.stride(0), int(zrows),
                                                             int(nr), int(p), ctypes.byref(rebuild), _ptr(out), out.stride(0), int(splits),
                                                             int(slab_stride), ctypes.byref(finalize) if finalize is not None else None,
                                                             ctypes.byref(xx) if xx is not None else None, self._stream()),
                   "vgan_mmd_backward_bf3_rm_rebuild")

    def mmd_backward_bf3_tile(self, nr, p, splits=1, tile=0):
        """Tile edge mmd_backward_bf3_rm runs for this shape (host-side query of the library's rule): a forced 64 / 128 / 256 as
        given; else 256 (256 x 128 tiles) once nr >= 256 and ceil(p / 128) * ceil(nr / 256) * splits >= 256; else 128 once
        ceil(p / 128) * ceil(nr / 128) * splits >= 512; else 64.  mmd_backward_bf3 (transposed images) runs 128 where this says 256."""
        return int(self.lib.vgan_mmd_backward_bf3_tile(int(nr), int(p), int(splits), int(tile)))

    def gemm_grouped(self, problems, copy=None, adadelta=None, noise=None, fold=None, kparts=None, ksplit_ws=None):
        """problems: up to 4 tuples (kind, A, B, C) with kind in "NN" (C = A.B), "NT" (C = A.B^T), "TN" (C = A^T.B); 2-D float32
        tensors with unit inner stride.  One launch; the products must not depend on each other.  A fifth tuple element
        `splits` > 1 cuts the contraction into that many slices run by different workgroups: C is then a contiguous
        [splits, m, n] tensor of partial products for the caller to sum (reduce_slabs).  Jobs that may ride in the launch
        (vgan_gemm_grouped_ex):
          copy = (src, dst)             contiguous float32 tensors of equal size, dst <- src;
          adadelta = dict(p, sq, acc, lr, rho, eps, weight_decay, grad_scale, layers=[(w_packed, off_w, off_b, out, in) per
                     problem (+ one more with extra_grad)], extra_grad=None): the optimiser update in the products' epilogue;
          noise = dict(next_noise, noise_cols, noise_ones_col, seed, step_counter): the next step's noise draw;
          fold = a finalize_job() run by one surplus workgroup (the late half of a split step tail).
        kparts = one count (1..8) per problem: that many workgroups share each 32 x 32 tile of the problem's contraction and
        combine inside the launch (vgan_gemm_grouped_ksplit; long-K launches on the 16-wave tiles only); `ksplit_ws` =
        ksplit_workspace(gemm_grouped_ksplit_ws_bytes(problems, kparts))."""
        assert 1 <= len(problems) <= _lib.GEMM_MAX_GROUP
        if kparts is not None and all(int(v) == 1 for v in kparts):
            kparts = None
        arr = self._gemm_problems(problems)
        if kparts is None and copy is None and adadelta is None and noise is None and fold is None:
            _lib.check(self.lib.vgan_gemm_grouped(arr, len(problems), self._stream()), "vgan_gemm_grouped")
            return
        x = self._grouped_extras(len(problems), copy, adadelta, noise, fold)
        if kparts is not None:
            assert len(kparts) == len(problems)
            kp = (ctypes.c_int32 * len(problems))(*[int(v) for v in kparts])
            _lib.check(self.lib.vgan_gemm_grouped_ksplit(arr, len(problems), ctypes.byref(x), kp, _ptr(ksplit_ws),
                                                         0 if ksplit_ws is None else ksplit_ws.numel() * ksplit_ws.element_size(),
                                                         self._stream()), "vgan_gemm_grouped_ksplit")
            return
        _lib.check(self.lib.vgan_gemm_grouped_ex(arr, len(problems), ctypes.byref(x), self._stream()), "vgan_gemm_grouped_ex")

    def gemm_grouped_path(self, problems, copy=None, adadelta=None, noise=None, fold=None, kparts=None):
        """(launch, [engine per problem]) gemm_grouped makes for exactly these arguments (lib.GEMM_GROUPED_PATHS /
        lib.GEMM_ENGINES; host-side query)."""
        if kparts is not None and all(int(v) == 1 for v in kparts):
            kparts = None
        arr = self._gemm_problems(problems)
        plain = copy is None and adadelta is None and noise is None and fold is None
        x = None if plain else ctypes.byref(self._grouped_extras(len(problems), copy, adadelta, noise, fold))
        kp = None if kparts is None else (ctypes.c_int32 * len(problems))(*[int(v) for v in kparts])
        engine = (ctypes.c_int32 * len(problems))()
        code = self.lib.vgan_gemm_grouped_path(arr, len(problems), x, kp, engine)
        return _lib.path_name(_lib.GEMM_GROUPED_PATHS, code, "vgan_gemm_grouped_path"), [_lib.GEMM_ENGINES[e] for e in engine]

    def gemm_grouped_ksplit_ws_bytes(self, problems, kparts):
        kp = (ctypes.c_int32 * len(problems))(*[int(v) for v in kparts])
        return int(self.lib.vgan_gemm_grouped_ksplit_ws_bytes(self._gemm_problems(problems), len(problems), kp))

    def _gemm_problems(self, problems):
        arr = (_lib.GemmProblem * len(problems))()
        for q, (kind, A, B, C, *rest) in zip(arr, problems):
            if kind == "NT2":  # C = (A . B^T) . D^T in one tile pass: (kind, A, B, C, D, scratch)
                D, scratch = rest
                _mat(A, "A"), _mat(B, "B"), _mat(C, "C"), _mat(D, "D")
                (m, k), (k2, kb), (n, k2d) = A.shape, B.shape, D.shape
                assert k == kb and k2 == k2d and tuple(C.shape) == (m, n)
                tiles = ((m + 63) // 64) * ((n + 63) // 64)
                assert scratch.is_cuda and scratch.dtype == _f32 and scratch.is_contiguous() and scratch.numel() >= tiles * 64 * _round4(k2)
                q.a, q.b, q.c, q.d, q.scratch = A.data_ptr(), B.data_ptr(), C.data_ptr(), D.data_ptr(), scratch.data_ptr()
                q.kind, q.m, q.n, q.k, q.k2, q.splitk = _lib.GEMM_NT_NT, m, n, k, k2, 1
                q.lda, q.ldb, q.ldc, q.ldd = A.stride(0), B.stride(0), C.stride(0), D.stride(0)
                continue
            q.splitk = int(rest[0]) if rest else 1
            if q.splitk > 1:
                assert C.dim() == 3 and C.shape[0] == q.splitk and C.is_contiguous()
                C = C[0]
            _mat(A, "A"), _mat(B, "B"), _mat(C, "C")
            if kind == "NN":
                (m, k), (k2, n), code = A.shape, B.shape, _lib.GEMM_NN
            elif kind == "NT":
                (m, k), (n, k2), code = A.shape, B.shape, _lib.GEMM_NT
            elif kind == "TN":
                (k, m), (k2, n), code = A.shape, B.shape, _lib.GEMM_TN
            else:
                raise ValueError(kind)
            assert k == k2 and tuple(C.shape) == (m, n), (kind, tuple(A.shape), tuple(B.shape), tuple(C.shape))
            q.a, q.b, q.c, q.kind, q.m, q.n, q.k = A.data_ptr(), B.data_ptr(), C.data_ptr(), code, m, n, k
            q.lda, q.ldb, q.ldc = A.stride(0), B.stride(0), C.stride(0)
        return arr

    def _grouped_extras(self, nproblems, copy, adadelta, noise, fold):
        x = _lib.GroupedExtras()
        if copy is not None:
            src, dst = copy
            _vec(src, "copy src"), _vec(dst, "copy dst")
            assert src.numel() == dst.numel()
            x.copy_src, x.copy_dst, x.copy_count = src.data_ptr(), dst.data_ptr(), src.numel()
        if adadelta is not None:
            a = adadelta
            for nm in ("p", "sq", "acc"):
                _vec(a[nm], nm)
            x.adadelta, x.p, x.sq_avg, x.acc_delta = 1, a["p"].data_ptr(), a["sq"].data_ptr(), a["acc"].data_ptr()
            x.lr, x.rho, x.eps, x.weight_decay, x.grad_scale = (float(a["lr"]), float(a.get("rho", 0.9)), float(a.get("eps", 1e-6)),
                                                                float(a.get("weight_decay", 0.0)), float(a.get("grad_scale", 1.0)))
            extra = a.get("extra_grad")
            assert len(a["layers"]) == nproblems + (1 if extra is not None else 0)
            for L, (w, off_w, off_b, out, inp) in zip(x.layer, a["layers"]):
                _mat(w, "w_packed")
                L.w_packed, L.off_w, L.off_b, L.ldp, L.out, L.inp = w.data_ptr(), int(off_w), int(off_b), w.stride(0), int(out), int(inp)
            if extra is not None:
                _mat(extra, "extra_grad")
                x.g_extra, x.ld_extra = extra.data_ptr(), extra.stride(0)
        if noise is not None:
            z = noise["next_noise"]
            x.next_noise, x.noise_rows, x.noise_ld = z.data_ptr(), z.shape[0], z.stride(0)
            x.noise_cols, x.noise_ones_col = int(noise["noise_cols"]), int(noise["noise_ones_col"])
            x.seed, x.step_counter = int(noise["seed"]) & 0xFFFFFFFFFFFFFFFF, noise["step_counter"].data_ptr()
        if fold is not None:
            x.fold = ctypes.addressof(fold)
        return x

    def mse_grad(self, target, pred, gscale, part, g):
        """part[ceil(n/4)] (float64) = partial sums of (pred - target)^2; g = gscale * (pred - target)."""
        _mat(target, "target"), _mat(pred, "pred"), _mat(g, "g")
        n, d = pred.shape
        assert part.dtype == torch.float64 and part.numel() >= (n + 3) // 4
        _lib.check(self.lib.vgan_mse_grad(_ptr(target), target.stride(0), _ptr(pred), pred.stride(0), n, d, float(gscale), _ptr(part),
                                          _ptr(g), g.stride(0), self._stream()), "vgan_mse_grad")

    def sum_f64(self, src, count, scale, out, accumulate=False):
        assert src.dtype == torch.float64
        _lib.check(self.lib.vgan_sum_f64(_ptr(src), int(count), float(scale), _ptr(out), int(bool(accumulate)), self._stream()),
                   "vgan_sum_f64")

    # ---- myopicity two-sample test -----------------------------------------------------------------
    def rbf_kernel_matrix(self, Z, sq, alpha, K):
        _mat(Z, "Z"), _mat(K, "K")
        m, p = Z.shape
        _lib.check(self.lib.vgan_rbf_kernel_matrix(_ptr(Z), Z.stride(0), m, p, _ptr(sq), float(alpha), _ptr(K), K.stride(0),
                                                   self._stream()), "vgan_rbf_kernel_matrix")

    def rows_dot(self, A, B, out, broadcast_b=False):
        """out[r] = <A[r], B[r]> (float64); broadcast_b: B is one row used for every r."""
        _mat(A, "A")
        rows, cols = A.shape
        assert out.dtype == torch.float64 and out.numel() >= rows
        ldb = 0 if broadcast_b else B.stride(0)
        _lib.check(self.lib.vgan_rows_dot(_ptr(A), A.stride(0), _ptr(B), ldb, _ptr(out), rows, cols, self._stream()), "vgan_rows_dot")

    # ---- data-parallel exchange through the C ABI (RCCL; the step engine itself uses torch.distributed) ------------
    def dp_unique_id(self):
        buf = (ctypes.c_uint8 * 128)()
        _lib.check(self.lib.vgan_dp_unique_id(ctypes.cast(buf, ctypes.c_void_p)), "vgan_dp_unique_id")
        return bytes(buf)

    def dp_comm_create(self, nranks, unique_id, rank):
        comm = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        _lib.check(self.lib.vgan_dp_comm_create(ctypes.byref(comm), int(nranks), ctypes.cast(buf, ctypes.c_void_p), int(rank)),
                   "vgan_dp_comm_create")
        return comm

    def dp_allreduce_sum(self, comm, t):
        _vec(t, "t")
        _lib.check(self.lib.vgan_dp_allreduce_sum(comm, _ptr(t), t.numel(), self._stream()), "vgan_dp_allreduce_sum")

    def dp_allgather(self, comm, t, nranks):
        """In-place all-gather over dim 0 of a contiguous tensor: rank r's slice is t[r * len(t) // nranks ...]."""
        assert t.is_cuda and t.is_contiguous() and t.shape[0] % nranks == 0
        _lib.check(self.lib.vgan_dp_allgather(comm, _ptr(t), t.numel() * t.element_size() // nranks, self._stream()), "vgan_dp_allgather")

    def dp_comm_destroy(self, comm):
        _lib.check(self.lib.vgan_dp_comm_destroy(comm), "vgan_dp_comm_destroy")

    # ---- input pipeline / sampling post-processing on the device ------------------------------------
    def shuffle_epoch(self, perm, train_size, seed, epoch):
        """perm (int32, any shape, contiguous): the first perm.numel() entries of a pseudo-random permutation of
        [0, train_size) keyed by (seed, epoch) -- one epoch of shuffled drop_last batches, produced on the device."""
        _vec(perm, "perm", torch.int32)
        _lib.check(self.lib.vgan_shuffle_epoch(_ptr(perm), perm.numel(), int(train_size), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               int(epoch) & 0xFFFFFFFFFFFFFFFF, self._stream()), "vgan_shuffle_epoch")

    def shuffle_index(self, i, train_size, seed, epoch):
        return int(self.lib.vgan_shuffle_index(int(i), int(train_size), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFFFFFFFFFF))

    def mask_unique(self, masks):
        """masks: bool [n, d] on the device -> (unique rows [m, d] bool in numpy's np.unique(axis=0) order, counts [m] int64)."""
        assert masks.is_cuda and masks.dtype == torch.bool and masks.dim() == 2
        m8 = masks.contiguous().view(torch.uint8)
        n, d = m8.shape
        dev = masks.device
        keys = torch.empty(n * ((d + 63) // 64), dtype=torch.int64, device=dev)
        work = torch.empty(2 * n, dtype=torch.int32, device=dev)
        out_row = torch.zeros(n, dtype=torch.int32, device=dev)
        out_count = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check(self.lib.vgan_mask_unique(_ptr(m8), m8.stride(0), n, d, _ptr(keys), _ptr(work), _ptr(out_row), _ptr(out_count),
                                             self._stream()), "vgan_mask_unique")
        cnt = out_count.cpu()
        m = int((cnt > 0).sum())
        return masks[out_row[:m].long()], cnt[:m].to(torch.int64)

    # ---- optimiser / noise / misc ----------------------------------------------------------------
    def adadelta_step(self, p, g, sq, acc, lr, rho=0.9, eps=1e-6, weight_decay=0.0, grad_scale=1.0, nslabs=1, slab_stride=0):
        """nslabs > 1: `g` is slab 0 of split-K gradient slabs `slab_stride` apart, summed inside the kernel."""
        for t, nm in ((p, "p"), (sq, "sq"), (acc, "acc")):
            _vec(t, nm)
        _lib.check(self.lib.vgan_adadelta_step(_ptr(p), _ptr(g), int(nslabs), int(slab_stride), _ptr(sq), _ptr(acc), p.numel(),
                                               float(lr), float(rho), float(eps),
                                               float(weight_decay), float(grad_scale), self._stream()), "vgan_adadelta_step")

    def adadelta_step_packed(self, p, pmap, g_packed, w_packed, sq, acc, lr, rho=0.9, eps=1e-6, weight_decay=0.0, grad_scale=1.0,
                             next_noise=None, noise_cols=0, noise_ones_col=-1, seed=0, step_counter=None):
        """next_noise [rows, ld]: also draw the next step's noise (first `noise_cols` columns, optional ones column)."""
        for t, nm in ((p, "p"), (sq, "sq"), (acc, "acc"), (g_packed, "g_packed"), (w_packed, "w_packed")):
            _vec(t, nm)
        _vec(pmap, "pmap", torch.int32)
        assert pmap.numel() == p.numel()
        zr, zld = (next_noise.shape[0], next_noise.stride(0)) if next_noise is not None else (0, 0)
        _lib.check(self.lib.vgan_adadelta_step_packed(_ptr(p), _ptr(pmap), _ptr(g_packed), _ptr(w_packed), _ptr(sq), _ptr(acc),
                                                      p.numel(), float(lr), float(rho), float(eps), float(weight_decay),
                                                      float(grad_scale), _ptr(next_noise), zr, int(noise_cols), zld,
                                                      int(noise_ones_col), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(step_counter),
                                                      self._stream()), "vgan_adadelta_step_packed")

    def noise_normal(self, z, seed, step_counter, stream_id=0, cols=None, ones_col=-1):
        """z [rows, ld]: standard normals in the first `cols` columns (default all); optional column of ones."""
        _mat(z, "z")
        rows, ld = z.shape[0], z.stride(0)
        cols = z.shape[1] if cols is None else int(cols)
        _lib.check(self.lib.vgan_noise_normal(_ptr(z), rows, cols, ld, int(ones_col), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              _ptr(step_counter), int(stream_id), self._stream()), "vgan_noise_normal")

    def homogeneous_pack(self, layers, unpack=False):
        """layers: [(W [out,in], b [out], P [>=out+1, >=in+1]) ...].  pack: P = [[W, b],[0, 1]]; unpack: (W, b) <- P.
        One launch for all layers; the device-side pointer table is built once per distinct layer set."""
        key = tuple((W.data_ptr(), tuple(W.shape), W.stride(0), b.data_ptr(), P.data_ptr(), tuple(P.shape), P.stride(0)) for W, b, P in layers)
        cache = self.__dict__.setdefault("_pack_tables", {})
        if key not in cache:
            if len(cache) >= 16:  # a handful of live engines at most: drop the oldest table instead of growing without bound
                cache.pop(next(iter(cache)))
            rows = []
            for W, b, P in layers:
                _mat(W, "W"), _vec(b, "b"), _mat(P, "P")
                out, kin = W.shape
                assert b.numel() == out and P.shape[0] >= out + 1 and P.shape[1] >= kin + 1
                rows.append([W.data_ptr(), b.data_ptr(), P.data_ptr(), out, kin, W.stride(0), P.stride(0), 0])
            cache[key] = (torch.tensor(rows, dtype=torch.int64, device=layers[0][0].device),
                          max((r[3] + 1) * (r[4] + 1) for r in rows))
        desc, max_elems = cache[key]
        _lib.check(self.lib.vgan_homogeneous_pack(_ptr(desc), desc.shape[0], int(max_elems), int(bool(unpack)), self._stream()),
                   "vgan_homogeneous_pack")

    def mse(self, a, b, scale, out, accumulate=False):
        _mat(a, "a"), _mat(b, "b")
        n, d = a.shape
        _lib.check(self.lib.vgan_mse(_ptr(a), a.stride(0), _ptr(b), b.stride(0), n, d, float(scale), _ptr(out),
                                     int(bool(accumulate)), self._stream()), "vgan_mse")

    # ---- outlier scoring over subspaces (vgan_amd.outlier) -------------------------------------------
    # A subspace table is (feat int32, feat_off int32 [S+1], col_off int64 [S+1]) on the device; calls cover [first, first + count).
    def outlier_pack(self, X, center, table, first, count, packed, sq=None):
        _mat(X, "X"), _vec(packed, "packed")
        feat, feat_off, col_off = table
        n, d = X.shape
        _lib.check(self.lib.vgan_outlier_pack(_ptr(X), X.stride(0), n, d, _ptr(center), _ptr(feat), _ptr(feat_off), _ptr(col_off),
                                              int(first), int(count), _ptr(packed), _ptr(sq), self._stream()), "vgan_outlier_pack")

    def outlier_knn(self, Pq, sq_q, nq, Pr, sq_r, nr, table, first, count, k, exclude_self, engine, splits, nbr,
                    part_d=None, part_i=None):
        _vec(nbr, "nbr", torch.int32)
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_outlier_knn(_ptr(Pq), _ptr(sq_q), int(nq), _ptr(Pr), _ptr(sq_r), int(nr), _ptr(feat_off), _ptr(col_off),
                                             int(first), int(count), int(k), int(bool(exclude_self)), int(engine), int(splits),
                                             _ptr(part_d), _ptr(part_i), _ptr(nbr), self._stream()), "vgan_outlier_knn")

    def outlier_refine(self, Xq, Xr, table, first, count, nbr, k, out_idx, out_dist, kdist=None):
        _mat(Xq, "Xq"), _mat(Xr, "Xr"), _vec(out_idx, "out_idx", torch.int32), _vec(out_dist, "out_dist")
        feat, feat_off, _ = table
        assert Xq.shape[1] == Xr.shape[1]
        _lib.check(self.lib.vgan_outlier_refine(_ptr(Xq), Xq.stride(0), Xq.shape[0], _ptr(Xr), Xr.stride(0), Xr.shape[0], Xq.shape[1],
                                                _ptr(feat), _ptr(feat_off), int(first), int(count), _ptr(nbr), int(k), _ptr(out_idx),
                                                _ptr(out_dist), _ptr(kdist), self._stream()), "vgan_outlier_refine")

    # The other metrics of the neighbour search (metric: VGAN_OUTLIER_METRIC_*, p: the Minkowski exponent, else unused)
    def outlier_pack_unit(self, X, table, first, count, packed, sq=None):
        _mat(X, "X"), _vec(packed, "packed")
        feat, feat_off, col_off = table
        n, d = X.shape
        _lib.check(self.lib.vgan_outlier_pack_unit(_ptr(X), X.stride(0), n, d, _ptr(feat), _ptr(feat_off), _ptr(col_off), int(first),
                                                   int(count), _ptr(packed), _ptr(sq), self._stream()), "vgan_outlier_pack_unit")

    def outlier_knn_metric(self, Pq, nq, Pr, nr, table, first, count, k, exclude_self, metric, p, splits, nbr, part_d=None,
                           part_i=None):
        _vec(nbr, "nbr", torch.int32)
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_outlier_knn_metric(_ptr(Pq), int(nq), _ptr(Pr), int(nr), _ptr(feat_off), _ptr(col_off), int(first),
                                                    int(count), int(k), int(bool(exclude_self)), int(metric), float(p), int(splits),
                                                    _ptr(part_d), _ptr(part_i), _ptr(nbr), self._stream()), "vgan_outlier_knn_metric")

    def outlier_refine_metric(self, Xq, Xr, table, first, count, nbr, k, metric, p, out_idx, out_dist, kdist=None):
        _mat(Xq, "Xq"), _mat(Xr, "Xr"), _vec(out_idx, "out_idx", torch.int32), _vec(out_dist, "out_dist")
        feat, feat_off, _ = table
        assert Xq.shape[1] == Xr.shape[1]
        _lib.check(self.lib.vgan_outlier_refine_metric(_ptr(Xq), Xq.stride(0), Xq.shape[0], _ptr(Xr), Xr.stride(0), Xr.shape[0],
                                                       Xq.shape[1], _ptr(feat), _ptr(feat_off), int(first), int(count), _ptr(nbr), int(k),
                                                       int(metric), float(p), _ptr(out_idx), _ptr(out_dist), _ptr(kdist), self._stream()),
                   "vgan_outlier_refine_metric")

    def outlier_score(self, idx, dist, nq, k, count, method, score=None, score_row=None, kdist_ref=None, lrd_ref=None, nr=0,
                      lrd_out=None):
        ld = score.stride(0) if score is not None else nq
        _lib.check(self.lib.vgan_outlier_score(_ptr(idx), _ptr(dist), int(nq), int(k), int(count), int(method), _ptr(kdist_ref),
                                               _ptr(lrd_ref), int(nr), _ptr(score), _ptr(score_row), int(ld), _ptr(lrd_out),
                                               self._stream()), "vgan_outlier_score")

    def outlier_kde(self, Pq, sq_q, nq, Pr, sq_r, nr, table, first, count, bandwidth, exclude_self, engine, splits, pivot, acc,
                    score, score_row=None):
        _vec(bandwidth, "bandwidth", torch.float64), _vec(pivot, "pivot", torch.int32), _vec(acc, "acc", torch.int64)
        _mat(score, "score")
        assert pivot.numel() >= count * nq and acc.numel() >= count * nq
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_outlier_kde(_ptr(Pq), _ptr(sq_q), int(nq), _ptr(Pr), _ptr(sq_r), int(nr), _ptr(feat_off), _ptr(col_off),
                                             int(first), int(count), _ptr(bandwidth), int(bool(exclude_self)), int(engine), int(splits),
                                             _ptr(pivot), _ptr(acc), _ptr(score), _ptr(score_row), score.stride(0), self._stream()),
                   "vgan_outlier_kde")

    def outlier_combine(self, score, weights, out):
        _mat(score, "score"), _vec(weights, "weights", torch.float64), _vec(out, "out", torch.float64)
        S, n = score.shape
        _lib.check(self.lib.vgan_outlier_combine(_ptr(score), score.stride(0), S, n, _ptr(weights), _ptr(out), self._stream()),
                   "vgan_outlier_combine")

    def outlier_abod(self, Xq, Xr, table, first, count, idx, k, score, score_row=None):
        """FastABOD scores of the refined lists idx [count, nq, k] into rows score_row of score; NaN marks a degenerate row."""
        _mat(Xq, "Xq"), _mat(Xr, "Xr"), _vec(idx, "idx", torch.int32), _mat(score, "score")
        feat, feat_off, _ = table
        assert Xq.shape[1] == Xr.shape[1] and idx.numel() >= count * Xq.shape[0] * k
        _lib.check(self.lib.vgan_outlier_abod(_ptr(Xq), Xq.stride(0), Xq.shape[0], _ptr(Xr), Xr.stride(0), Xr.shape[0], Xq.shape[1],
                                              _ptr(feat), _ptr(feat_off), int(first), int(count), _ptr(idx), int(k), _ptr(score),
                                              _ptr(score_row), score.stride(0), self._stream()), "vgan_outlier_abod")

    def _outlier_fill_degenerate(self, name, score, value, n_degenerate):
        _mat(score, "score"), _vec(value, "value", torch.float64)
        S, n = score.shape
        assert value.numel() >= S
        if n_degenerate is not None:
            _vec(n_degenerate, "n_degenerate", torch.int32)
            assert n_degenerate.numel() >= S
        _lib.check(getattr(self.lib, name)(_ptr(score), score.stride(0), S, n, int(n_degenerate is not None), _ptr(value),
                                           _ptr(n_degenerate), self._stream()), name)

    def outlier_abod_floor(self, score, score_floor, n_degenerate=None):
        """n_degenerate given (fit): score_floor [S] and n_degenerate [S] are taken from score [S, n]; otherwise score_floor
        is applied as stored.  Either way the NaN scores of row s become score_floor[s]."""
        self._outlier_fill_degenerate("vgan_outlier_abod_floor", score, score_floor, n_degenerate)

    def outlier_cof_chain(self, Xq, Xr, table, first, count, idx, k, chain, ac_out):
        """Average chaining distances (COF) of the refined lists idx [count, nq, k] into ac_out, float64 [count, nq]; chain is
        a VGAN_OUTLIER_COF_CHAIN_* value."""
        _mat(Xq, "Xq"), _mat(Xr, "Xr"), _vec(idx, "idx", torch.int32), _vec(ac_out, "ac_out", torch.float64)
        feat, feat_off, _ = table
        assert Xq.shape[1] == Xr.shape[1] and idx.numel() >= count * Xq.shape[0] * k and ac_out.numel() >= count * Xq.shape[0]
        _lib.check(self.lib.vgan_outlier_cof_chain(_ptr(Xq), Xq.stride(0), Xq.shape[0], _ptr(Xr), Xr.stride(0), Xr.shape[0],
                                                   Xq.shape[1], _ptr(feat), _ptr(feat_off), int(first), int(count), _ptr(idx), int(k),
                                                   int(chain), _ptr(ac_out), self._stream()), "vgan_outlier_cof_chain")

    def outlier_cof_score(self, ac_q, ac_ref, idx, k, score, score_row=None):
        """COF scores ac_q k / sum ac_ref[idx] of the lists idx [count, nq, k] (ac_q [count, nq], ac_ref [count, nr], float64,
        contiguous) into rows score_row of score; NaN marks a degenerate row."""
        _vec(ac_q, "ac_q", torch.float64), _vec(ac_ref, "ac_ref", torch.float64), _vec(idx, "idx", torch.int32), _mat(score, "score")
        assert ac_q.dim() == 2 and ac_ref.dim() == 2 and ac_q.shape[0] == ac_ref.shape[0]
        count, nq = ac_q.shape
        assert idx.numel() >= count * nq * k
        _lib.check(self.lib.vgan_outlier_cof_score(_ptr(ac_q), nq, _ptr(ac_ref), ac_ref.shape[1], _ptr(idx), int(k), count, _ptr(score),
                                                   _ptr(score_row), score.stride(0), self._stream()), "vgan_outlier_cof_score")

    def outlier_cof_ceiling(self, score, score_ceiling, n_degenerate=None):
        """outlier_abod_floor with a maximum: n_degenerate given (fit) takes score_ceiling [S] and n_degenerate [S] from score
        [S, n]; either way the NaN scores of row s become score_ceiling[s]."""
        self._outlier_fill_degenerate("vgan_outlier_cof_ceiling", score, score_ceiling, n_degenerate)

    def outlier_score_stats(self, score, mode, center, scale):
        """center / scale (float64 [S]) of the rows of score [S, n]; mode is a VGAN_OUTLIER_NORM_* value."""
        _mat(score, "score"), _vec(center, "center", torch.float64), _vec(scale, "scale", torch.float64)
        S, n = score.shape
        assert center.numel() >= S and scale.numel() >= S
        need = self.lib.vgan_outlier_score_stats_ws_bytes(S, n, int(mode))
        if need < 0:
            _lib.check(1, "vgan_outlier_score_stats_ws_bytes")
        ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=score.device)
        _lib.check(self.lib.vgan_outlier_score_stats(_ptr(score), score.stride(0), S, n, int(mode), _ptr(center), _ptr(scale),
                                                     _ptr(ws), ws.numel() * 8, self._stream()), "vgan_outlier_score_stats")

    def outlier_combine_normalized(self, score, center, scale, weights, combination, out):
        """out[i] = sum_s weights[s] t_s or max_s t_s with t_s = (score[s, i] - center[s]) / scale[s] (center / scale None:
        the raw scores); combination is a VGAN_OUTLIER_COMBINE_* value."""
        _mat(score, "score"), _vec(out, "out", torch.float64)
        for name, v in (("center", center), ("scale", scale), ("weights", weights)):
            if v is not None:
                _vec(v, name, torch.float64)
        S, n = score.shape
        _lib.check(self.lib.vgan_outlier_combine_normalized(_ptr(score), score.stride(0), S, n, _ptr(center), _ptr(scale),
                                                            _ptr(weights), int(combination), _ptr(out), self._stream()),
                   "vgan_outlier_combine_normalized")

    # ---- k-means / CBLOF over subspaces (vgan_amd.outlier.SubspaceCBLOF) ------------------------------
    def cluster_lloyd_ws_bytes(self, n, n_clusters, count, total_dims):
        need = self.lib.vgan_cluster_lloyd_ws_bytes(int(n), int(n_clusters), int(count), int(total_dims))
        if need < 0:
            _lib.check(1, "vgan_cluster_lloyd_ws_bytes")
        return need

    def cluster_image(self, centers, n_clusters, table, first, count, col_center, img, img_sq=None):
        _vec(centers, "centers", torch.float64), _vec(img, "img")
        feat, feat_off, col_off = table
        _lib.check(self.lib.vgan_cluster_image(_ptr(centers), int(n_clusters), _ptr(feat), _ptr(feat_off), _ptr(col_off), int(first),
                                               int(count), _ptr(col_center), _ptr(img), _ptr(img_sq), self._stream()),
                   "vgan_cluster_image")

    def cluster_lloyd(self, Pq, sq_q, X, table, first, count, total_dims, max_dims, n_clusters, engine, col_center, tol_var, centers,
                      img, img_sq, label, changed, done, n_iter, workspace, iterations):
        """Enqueues `iterations` Lloyd iterations for the chunk [first, first + count); reads nothing back."""
        _mat(X, "X"), _vec(Pq, "Pq"), _vec(img, "img"), _vec(centers, "centers", torch.float64), _vec(tol_var, "tol_var", torch.float64)
        _vec(workspace, "workspace", torch.float64), _vec(label, "label", torch.int32)
        for name, v in (("changed", changed), ("done", done), ("n_iter", n_iter)):
            _vec(v, name, torch.int32)
        assert label.numel() >= count * X.shape[0]
        feat, feat_off, col_off = table
        n, d = X.shape
        _lib.check(self.lib.vgan_cluster_lloyd(_ptr(Pq), _ptr(sq_q), _ptr(X), X.stride(0), n, d, _ptr(feat), _ptr(feat_off), _ptr(col_off),
                                               int(first), int(count), int(total_dims), int(max_dims), int(n_clusters), int(engine),
                                               _ptr(col_center), _ptr(tol_var), _ptr(centers), _ptr(img), _ptr(img_sq), _ptr(label),
                                               _ptr(changed), _ptr(done), _ptr(n_iter), _ptr(workspace), workspace.numel() * 8,
                                               int(iterations), self._stream()), "vgan_cluster_lloyd")

    def cluster_final(self, Xq, table, S, n_clusters, centers, sizes, large=None, use_weights=False, label=None, inertia=None,
                      score=None, score_row=None):
        """large None: label [S, nq], sizes [S, C] (+=) and inertia [S]; otherwise the CBLOF scores (and label if given)."""
        _mat(Xq, "Xq"), _vec(centers, "centers", torch.float64), _vec(sizes, "sizes", torch.int64)
        feat, feat_off, _ = table
        nq, d = Xq.shape
        part = None
        if large is None:
            _vec(label, "label", torch.int32), _vec(inertia, "inertia", torch.float64)
            assert label.numel() >= S * nq and inertia.numel() >= S
            part = torch.empty(S * ((nq + 63) // 64), dtype=torch.float64, device=Xq.device)
        else:
            _vec(large, "large", torch.int32), _mat(score, "score")
            assert large.numel() >= S * n_clusters and score.shape[0] >= S
        assert sizes.numel() >= S * n_clusters
        _lib.check(self.lib.vgan_cluster_final(_ptr(Xq), Xq.stride(0), nq, d, _ptr(feat), _ptr(feat_off), int(S), int(n_clusters),
                                               _ptr(centers), _ptr(large), _ptr(sizes), int(bool(use_weights)), _ptr(label), _ptr(part),
                                               _ptr(inertia), _ptr(score), _ptr(score_row), score.stride(0) if score is not None else 0,
                                               self._stream()), "vgan_cluster_final")


    # ---- ECOD over subspaces (vgan_amd.outlier.SubspaceECOD) ------------------------------------------------
    def ecod_sort_columns(self, X, sorted_cols):
        """sorted_cols float32 [d, n_pad] (n_pad the power of two with n <= n_pad < 2 n): the ascending columns of X [n, d]."""
        _mat(X, "X"), _vec(sorted_cols, "sorted_cols")
        n, d = X.shape
        assert sorted_cols.dim() == 2 and sorted_cols.shape[0] == d
        _lib.check(self.lib.vgan_ecod_sort_columns(_ptr(X), X.stride(0), n, d, _ptr(sorted_cols), sorted_cols.shape[1], self._stream()),
                   "vgan_ecod_sort_columns")

    def ecod_skew_sign(self, sorted_cols, n, sign):
        """sign int8 [d]: the skewness sign of the first n entries of every row of sorted_cols [d, ld]."""
        _vec(sorted_cols, "sorted_cols"), _vec(sign, "sign", torch.int8)
        d, ld = sorted_cols.shape
        assert sign.numel() >= d
        _lib.check(self.lib.vgan_ecod_skew_sign(_ptr(sorted_cols), ld, int(n), d, _ptr(sign), self._stream()), "vgan_ecod_skew_sign")

    def ecod_tail_counts(self, Xq, sorted_cols, n, cl, cr):
        """cl / cr int32 [rows, d]: how many of the n fitted values of each feature are <= / >= the query value."""
        _mat(Xq, "Xq"), _vec(sorted_cols, "sorted_cols"), _vec(cl, "cl", torch.int32), _vec(cr, "cr", torch.int32)
        rows, d = Xq.shape
        assert sorted_cols.shape[0] == d and cl.numel() >= rows * d and cr.numel() >= rows * d
        _lib.check(self.lib.vgan_ecod_tail_counts(_ptr(Xq), Xq.stride(0), rows, d, _ptr(sorted_cols), sorted_cols.shape[1], int(n),
                                                  _ptr(cl), _ptr(cr), self._stream()), "vgan_ecod_tail_counts")

    def ecod_scores(self, cl, cr, rows, sign, n, query, aggregate, mask, terms, score):
        """score float32 [S, rows] (a view into the score matrix may be given) from the counts of `rows` rows; mask float64
        [d, S]; terms: float64 workspace of rows * d (aggregate 0) or 3 * rows * d (aggregate 1) elements."""
        _vec(cl, "cl", torch.int32), _vec(cr, "cr", torch.int32), _vec(sign, "sign", torch.int8), _mat(score, "score")
        _vec(mask, "mask", torch.float64), _vec(terms, "terms", torch.float64)
        d, S = mask.shape
        assert cl.numel() >= rows * d and cr.numel() >= rows * d and sign.numel() >= d
        assert terms.numel() >= (3 if aggregate else 1) * rows * d and score.shape[0] == S and score.shape[1] >= rows
        _lib.check(self.lib.vgan_ecod_scores(_ptr(cl), _ptr(cr), int(rows), d, _ptr(sign), int(n), int(bool(query)), int(aggregate),
                                             _ptr(mask), S, S, _ptr(terms), _ptr(score), score.stride(0), self._stream()),
                   "vgan_ecod_scores")

    # ---- HiCS subspace contrast (vgan_amd.hics) ---------------------------------------------------------------
    def hics_argsort_columns(self, X, keys, order, rank):
        """order / rank int32 [d, n] (read as uint32): the stable ascending order of every column of X [n, d] and its inverse;
        keys: int64 workspace [d, n_pad], n_pad the power of two with n <= n_pad < 2 n."""
        _mat(X, "X"), _vec(keys, "keys", torch.int64), _vec(order, "order", torch.int32), _vec(rank, "rank", torch.int32)
        n, d = X.shape
        assert keys.dim() == 2 and keys.shape[0] == d and order.numel() >= n * d and rank.numel() >= n * d
        _lib.check(self.lib.vgan_hics_argsort_columns(_ptr(X), X.stride(0), n, d, _ptr(keys), keys.shape[1], _ptr(order), _ptr(rank),
                                                      self._stream()), "vgan_hics_argsort_columns")

    def hics_contrast(self, order, rank, feat, feat_off, width, stream_id, S, M, seed, D, m, c, contrast, n_empty, group=0):
        """The draws (D int64, m / c int32 [S, M]), contrasts (float64 [S]) and empty-draw counts (int32 [S]) of the S
        subspaces whose offsets start at feat_off[0]; width int32 [S], stream_id int64 [S] (read as uint64)."""
        _vec(order, "order", torch.int32), _vec(rank, "rank", torch.int32), _vec(feat, "feat", torch.int32)
        _vec(feat_off, "feat_off", torch.int32), _vec(width, "width", torch.int32), _vec(stream_id, "stream_id", torch.int64)
        _vec(D, "D", torch.int64), _vec(m, "m", torch.int32), _vec(c, "c", torch.int32)
        _vec(contrast, "contrast", torch.float64), _vec(n_empty, "n_empty", torch.int32)
        d, n = order.shape
        assert rank.shape == order.shape and feat_off.numel() >= S + 1 and width.numel() >= S and stream_id.numel() >= S
        assert min(D.numel(), m.numel(), c.numel()) >= S * M and contrast.numel() >= S and n_empty.numel() >= S
        _lib.check(self.lib.vgan_hics_contrast(_ptr(order), _ptr(rank), n, d, _ptr(feat), _ptr(feat_off), _ptr(width), _ptr(stream_id),
                                               int(S), int(M), int(seed) & (2 ** 64 - 1), int(group), _ptr(D), _ptr(m), _ptr(c),
                                               _ptr(contrast), _ptr(n_empty), self._stream()), "vgan_hics_contrast")

    # ---- histogram scores over subspaces (vgan_amd.outlier.SubspaceHBOS / SubspaceLODA) ----------------------
    # keys: int64 [P, 2] holding the library's uint64 order-preserving keys of a column's minimum and maximum
    def hist_column_range(self, X, keys):
        """keys [d, 2]: the keys of the minimum and maximum of every column of X [n, d] (set first: nothing is merged)."""
        _mat(X, "X"), _vec(keys, "keys", torch.int64)
        n, d = X.shape
        assert keys.numel() >= 2 * d
        _lib.check(self.lib.vgan_hist_column_range(_ptr(X), X.stride(0), n, d, _ptr(keys), self._stream()), "vgan_hist_column_range")

    def hist_edges(self, keys, n_bins, edges):
        """edges float64 [P, n_bins + 1] = numpy.linspace(lo, hi, n_bins + 1) of every column's range (lo == hi: +-0.5)."""
        _vec(keys, "keys", torch.int64), _vec(edges, "edges", torch.float64)
        P = edges.numel() // (int(n_bins) + 1)
        assert edges.numel() == P * (int(n_bins) + 1) and keys.numel() >= 2 * P
        _lib.check(self.lib.vgan_hist_edges(_ptr(keys), P, int(n_bins), _ptr(edges), self._stream()), "vgan_hist_edges")

    def hist_column_counts(self, X, edges, counts):
        """counts int32 [d, B] (zeroed first): how many values of every column of X [n, d] fall into each bin of edges
        float64 [d, B + 1]."""
        _mat(X, "X"), _vec(edges, "edges", torch.float64), _vec(counts, "counts", torch.int32)
        n, d = X.shape
        B = edges.shape[-1] - 1
        assert edges.numel() == d * (B + 1) and counts.numel() >= d * B
        _lib.check(self.lib.vgan_hist_column_counts(_ptr(X), X.stride(0), n, d, _ptr(edges), B, _ptr(counts), self._stream()),
                   "vgan_hist_column_counts")

    def hbos_scores(self, Xq, edges, table, limits, mask, terms, score):
        """score float32 [S, rows] (a view into the score matrix may be given) of the rows of Xq: the masked sums of the
        looked-up terms; table float64 [d, B + 1], limits float64 [d, 2], mask float64 [d, S]; terms: float64 workspace of
        rows * d elements."""
        _mat(Xq, "Xq"), _mat(score, "score")
        for name, t in (("edges", edges), ("table", table), ("limits", limits), ("mask", mask), ("terms", terms)):
            _vec(t, name, torch.float64)
        rows, d = Xq.shape
        B = edges.shape[-1] - 1
        S = mask.shape[1]
        assert edges.numel() == d * (B + 1) and table.numel() == d * (B + 1) and limits.numel() == 2 * d and mask.shape[0] == d
        assert terms.numel() >= rows * d and score.shape[0] == S and score.shape[1] >= rows
        _lib.check(self.lib.vgan_hbos_scores(_ptr(Xq), Xq.stride(0), rows, d, _ptr(edges), B, _ptr(table), _ptr(limits), _ptr(mask), S, S,
                                             _ptr(terms), _ptr(score), score.stride(0), self._stream()), "vgan_hbos_scores")

    def hist_reset(self, keys=None, counts=None):
        """keys to (above every key, below every key) and counts to 0, before the LODA calls that merge into them."""
        if keys is not None:
            _vec(keys, "keys", torch.int64)
        if counts is not None:
            _vec(counts, "counts", torch.int32)
        _lib.check(self.lib.vgan_hist_reset(_ptr(keys), 0 if keys is None else keys.numel() // 2, _ptr(counts),
                                            0 if counts is None else counts.numel(), self._stream()), "vgan_hist_reset")

    # packed: the packed block (outlier_pack, not centred) of `rows` rows for the subspaces first .. first + count - 1;
    # proj: (pidx int32, pw float64, moff int64 [S + 1], k): the projections' nonzeros, t-major per subspace
    def loda_range(self, packed, rows, table, first, count, max_dims, proj, keys):
        """Merges the keys of the projected values of the block's rows into keys [S, k, 2]."""
        _vec(packed, "packed"), _vec(keys, "keys", torch.int64)
        _, feat_off, col_off = table
        pidx, pw, moff, k = proj
        assert keys.numel() >= 2 * (first + count) * k
        _lib.check(self.lib.vgan_loda_range(_ptr(packed), int(rows), _ptr(feat_off), _ptr(col_off), int(first), int(count), int(max_dims),
                                            _ptr(pidx), _ptr(pw), _ptr(moff), int(k), _ptr(keys), self._stream()), "vgan_loda_range")

    def loda_counts(self, packed, rows, table, first, count, max_dims, proj, edges, counts):
        """Adds the bins of the projected values of the block's rows to counts int32 [S, k, B]; edges float64 [S, k, B + 1]."""
        _vec(packed, "packed"), _vec(edges, "edges", torch.float64), _vec(counts, "counts", torch.int32)
        _, feat_off, col_off = table
        pidx, pw, moff, k = proj
        B = edges.shape[-1] - 1
        assert edges.numel() >= (first + count) * k * (B + 1) and counts.numel() >= (first + count) * k * B
        _lib.check(self.lib.vgan_loda_counts(_ptr(packed), int(rows), _ptr(feat_off), _ptr(col_off), int(first), int(count), int(max_dims),
                                             _ptr(pidx), _ptr(pw), _ptr(moff), int(k), _ptr(edges), B, _ptr(counts), self._stream()),
                   "vgan_loda_counts")

    def loda_scores(self, packed, rows, table, first, count, max_dims, proj, edges, terms, score):
        """score float32 [S, rows] (a view into the score matrix, all S rows of it): rows first .. first + count - 1 receive
        the mean of terms float64 [S, k, B] at the bins of the projected values."""
        _vec(packed, "packed"), _vec(edges, "edges", torch.float64), _vec(terms, "terms", torch.float64), _mat(score, "score")
        _, feat_off, col_off = table
        pidx, pw, moff, k = proj
        B = edges.shape[-1] - 1
        assert edges.numel() >= (first + count) * k * (B + 1) and terms.numel() >= (first + count) * k * B
        assert score.shape[0] >= first + count and score.shape[1] >= rows
        _lib.check(self.lib.vgan_loda_scores(_ptr(packed), int(rows), _ptr(feat_off), _ptr(col_off), int(first), int(count), int(max_dims),
                                             _ptr(pidx), _ptr(pw), _ptr(moff), int(k), _ptr(edges), B, _ptr(terms), _ptr(score),
                                             score.stride(0), self._stream()), "vgan_loda_scores")

    # ---- isolation forest over subspaces (vgan_amd.outlier.SubspaceIForest) ---------------------------------
    def iforest_build(self, X, table, first, count, max_dims, psi, depth, seed, nodes):
        """nodes int32 [S, T, N, 2] (N = 2^(depth + 1)) receives the T trees of the subspaces first .. first + count - 1,
        built from X [n, d] on psi sampled rows each; max_dims: the most features of a subspace of the range."""
        _mat(X, "X"), _vec(nodes, "nodes", torch.int32)
        feat, feat_off, _ = table
        n, d = X.shape
        S, T = nodes.shape[:2]
        assert nodes.dim() == 4 and nodes.shape[2] == 2 << depth and nodes.shape[3] == 2 and first + count <= S
        _lib.check(self.lib.vgan_iforest_build(_ptr(X), X.stride(0), n, d, _ptr(feat), _ptr(feat_off), int(first), int(count),
                                               int(max_dims), T, int(psi), int(depth), int(seed), _ptr(nodes), self._stream()),
                   "vgan_iforest_build")

    def iforest_path_sums(self, Xq, nodes, first, count, psi, depth, cq, sums):
        """sums int64 [count, rows]: per query row of Xq and subspace of the range, the fixed-point path lengths summed over
        the subspace's trees; cq int64 [psi + 1]: the Q32 average path lengths."""
        _mat(Xq, "Xq"), _vec(nodes, "nodes", torch.int32), _vec(cq, "cq", torch.int64), _vec(sums, "sums", torch.int64)
        rows, d = Xq.shape
        S, T = nodes.shape[:2]
        assert nodes.dim() == 4 and nodes.shape[2] == 2 << depth and nodes.shape[3] == 2 and first + count <= S
        assert cq.numel() >= psi + 1 and sums.numel() >= count * rows
        _lib.check(self.lib.vgan_iforest_path_sums(_ptr(Xq), Xq.stride(0), rows, d, _ptr(nodes), int(first), int(count), T, int(psi),
                                                   int(depth), _ptr(cq), _ptr(sums), rows, self._stream()), "vgan_iforest_path_sums")

    def iforest_scores(self, sums, count, rows, denom, score):
        """score float32 [count, rows] (a view into the score matrix may be given) = exp2(-sums / denom)."""
        _vec(sums, "sums", torch.int64), _mat(score, "score")
        assert sums.numel() >= count * rows and score.shape[0] == count and score.shape[1] >= rows
        _lib.check(self.lib.vgan_iforest_scores(_ptr(sums), int(rows), int(count), int(rows), int(denom), _ptr(score), score.stride(0),
                                                self._stream()), "vgan_iforest_scores")

    def iforest_build_oblique(self, X, cand, cand_off, first, count, psi, depth, seed, nodes, plane_col, plane_w):
        """nodes int32 [S, T, N, 2], plane_col int32 and plane_w float32 [S, T, N, q] receive the T oblique trees of the
        subspaces first .. first + count - 1, built from the dense X [n, d]; cand int32: the candidate columns of every
        subspace, concatenated, cand_off int32 [S + 1] their offsets."""
        _vec(X, "X"), _vec(nodes, "nodes", torch.int32), _vec(plane_col, "plane_col", torch.int32), _vec(plane_w, "plane_w")
        _vec(cand, "cand", torch.int32), _vec(cand_off, "cand_off", torch.int32)
        n, d = X.shape
        S, T, N, q = plane_col.shape
        assert tuple(nodes.shape) == (S, T, N, 2) and plane_w.shape == plane_col.shape and N == 2 << depth and first + count <= S
        assert cand_off.numel() == S + 1
        _lib.check(self.lib.vgan_iforest_build_oblique(_ptr(X), n, d, _ptr(cand), _ptr(cand_off), int(first), int(count), T, int(psi),
                                                       int(depth), q, int(seed), _ptr(nodes), _ptr(plane_col), _ptr(plane_w),
                                                       self._stream()), "vgan_iforest_build_oblique")

    def iforest_path_sums_oblique(self, Xq, nodes, plane_col, plane_w, first, count, psi, depth, cq, sums):
        """sums int64 [count, rows]: iforest_path_sums through oblique trees; Xq [rows, d] dense."""
        _vec(Xq, "Xq"), _vec(nodes, "nodes", torch.int32), _vec(plane_col, "plane_col", torch.int32), _vec(plane_w, "plane_w")
        _vec(cq, "cq", torch.int64), _vec(sums, "sums", torch.int64)
        rows, d = Xq.shape
        S, T, N, q = plane_col.shape
        assert tuple(nodes.shape) == (S, T, N, 2) and plane_w.shape == plane_col.shape and N == 2 << depth and first + count <= S
        assert cq.numel() >= psi + 1 and sums.numel() >= count * rows
        _lib.check(self.lib.vgan_iforest_path_sums_oblique(_ptr(Xq), rows, d, _ptr(nodes), _ptr(plane_col), _ptr(plane_w), int(first),
                                                           int(count), T, int(psi), int(depth), q, _ptr(cq), _ptr(sums), rows,
                                                           self._stream()), "vgan_iforest_path_sums_oblique")

    def iforest_build_blocks(self, R, first, psi, depth, seed, nodes):
        """nodes int32 [blocks, T, N, 2] receives the T trees of the blocks first .. first + count - 1, block first + z grown
        on its own matrix R[z] of R float32 [count, n, q] (every column a candidate); stream id = block T + tree."""
        _vec(R, "R"), _vec(nodes, "nodes", torch.int32)
        count, n, q = R.shape
        B, T = nodes.shape[:2]
        assert nodes.dim() == 4 and nodes.shape[2] == 2 << depth and nodes.shape[3] == 2 and first + count <= B
        _lib.check(self.lib.vgan_iforest_build_blocks(_ptr(R), n * q, n, q, int(first), count, T, int(psi), int(depth), int(seed),
                                                      _ptr(nodes), self._stream()), "vgan_iforest_build_blocks")

    def iforest_path_sums_blocks(self, Rq, nodes, first, psi, depth, cq, sums):
        """sums int64 [count, rows]: the rows of Rq float32 [count, rows, q], block by block, walked through the trees of the
        blocks first .. first + count - 1."""
        _vec(Rq, "Rq"), _vec(nodes, "nodes", torch.int32), _vec(cq, "cq", torch.int64), _vec(sums, "sums", torch.int64)
        count, rows, q = Rq.shape
        B, T = nodes.shape[:2]
        assert nodes.dim() == 4 and nodes.shape[2] == 2 << depth and nodes.shape[3] == 2 and first + count <= B
        assert cq.numel() >= psi + 1 and sums.numel() >= count * rows
        _lib.check(self.lib.vgan_iforest_path_sums_blocks(_ptr(Rq), rows * q, rows, q, _ptr(nodes), int(first), count, T, int(psi),
                                                          int(depth), _ptr(cq), _ptr(sums), rows, self._stream()),
                   "vgan_iforest_path_sums_blocks")

    # ---- RS-Hash grid counts over subspaces (vgan_amd.outlier.SubspaceRSHash) -------------------------------
    # comp: (dims int32 [S, T], feat int32 [S, T, 12], shift float64 [S, T, 12], width float64 [S, T]): the host's draws;
    # state: (cell_key int64 [S, T, s] holding the library's uint64 keys, cell_count int32 [S, T, s], n_cells int32 [S, T],
    # sample_min float32 [S, T, 12], sample_max float32 [S, T, 12])
    @staticmethod
    def _rshash_tables(comp, state):
        dims, feat, shift, width = comp
        key, cnt, cells, lo, hi = state
        S, T, s = key.shape
        _vec(dims, "comp dims", torch.int32), _vec(feat, "comp feat", torch.int32)
        _vec(shift, "comp shift", torch.float64), _vec(width, "comp width", torch.float64)
        _vec(key, "cell_key", torch.int64), _vec(cnt, "cell_count", torch.int32), _vec(cells, "n_cells", torch.int32)
        _vec(lo, "sample_min"), _vec(hi, "sample_max")
        assert dims.numel() == S * T and width.numel() == S * T and cells.numel() == S * T and cnt.numel() == S * T * s
        assert min(feat.numel(), shift.numel(), lo.numel(), hi.numel()) >= S * T * 12
        return S, T, s

    def rshash_build(self, X, first, count, seed, comp, state, sample_rows=None):
        """Fills the state of the components of the subspaces first .. first + count - 1 from X [n, d]; sample_rows int32
        [S, T, s] (optional) receives every component's sorted sample."""
        _mat(X, "X")
        S, T, s = self._rshash_tables(comp, state)
        n, d = X.shape
        assert first + count <= S
        if sample_rows is not None:
            _vec(sample_rows, "sample_rows", torch.int32)
            assert sample_rows.numel() == S * T * s
        _lib.check(self.lib.vgan_rshash_build(_ptr(X), X.stride(0), n, d, int(first), int(count), T, s, int(seed), *map(_ptr, comp),
                                              *map(_ptr, state), _ptr(sample_rows), self._stream()), "vgan_rshash_build")

    def rshash_cell_sums(self, Xq, column_major, row_base, first, count, comp, state, sample_rows, table, sums):
        """sums int64 [count, rows]: per query row and subspace of the range, table[c] summed over the subspace's components.
        Xq: float32 [rows, d], or with column_major its transposed copy [d, rows] (a column slice of one may be given);
        sample_rows: the fit's sorted samples (its rows are rows row_base .. of the fitted X), None for new rows."""
        _mat(Xq if Xq.shape[1] > 1 else Xq[:, 0:1].as_strided(Xq.shape, (Xq.stride(0), 1)), "Xq")  # a single column has no inner stride
        _vec(table, "table", torch.int64), _vec(sums, "sums", torch.int64)
        S, T, s = self._rshash_tables(comp, state)
        d, rows = Xq.shape if column_major else Xq.shape[::-1]
        strides = (1, Xq.stride(0)) if column_major else (Xq.stride(0), 1)
        assert first + count <= S and table.numel() >= s + 2 and sums.numel() >= count * rows
        if sample_rows is not None:
            _vec(sample_rows, "sample_rows", torch.int32)
            assert sample_rows.numel() == S * T * s
        _lib.check(self.lib.vgan_rshash_cell_sums(_ptr(Xq), *strides, rows, d, int(row_base), int(first), int(count), T, s,
                                                  *map(_ptr, comp), *map(_ptr, state), _ptr(sample_rows), _ptr(table), _ptr(sums), rows,
                                                  self._stream()), "vgan_rshash_cell_sums")

    def rshash_scores(self, sums, count, rows, denom, score):
        """score float32 [count, rows] (a view into the score matrix may be given) = 1 - sums / denom."""
        _vec(sums, "sums", torch.int64), _mat(score, "score")
        assert sums.numel() >= count * rows and score.shape[0] == count and score.shape[1] >= rows
        _lib.check(self.lib.vgan_rshash_scores(_ptr(sums), int(rows), int(count), int(rows), int(denom), _ptr(score), score.stride(0),
                                               self._stream()), "vgan_rshash_scores")

    # ---- deep isolation forest over subspaces (vgan_amd.outlier.SubspaceDIF) --------------------------------
    # net: (r, hidden tuple, q, activation code); w_off: int64 [count] on the device, the blocks' offsets into W
    def dif_weights(self, feat_off, net, first, count, scale, seed, W, w_off, total):
        """W float32 [>= total]: zeroed, then the Philox weights of the blocks first .. first + count - 1 (layer l of a block
        quad-major as [round8(K_l) / 4][K_{l+1}][4]); scale float64 [S, layers]: c_l = 1 / sqrt(K_l) per subspace."""
        _vec(feat_off, "feat_off", torch.int32), _vec(scale, "scale", torch.float64), _vec(W, "W"), _vec(w_off, "w_off", torch.int64)
        r, hidden, q, _ = net
        assert W.numel() >= total and w_off.numel() >= count and scale.numel() >= (feat_off.numel() - 1) * (len(hidden) + 1)
        assert (first + count - 1) // r < feat_off.numel() - 1
        harr = (ctypes.c_int32 * max(len(hidden), 1))(*hidden)
        _lib.check(self.lib.vgan_dif_weights(_ptr(feat_off), int(r), int(first), int(count), len(hidden), harr, int(q), _ptr(scale),
                                             int(seed), _ptr(W), _ptr(w_off), int(total), self._stream()), "vgan_dif_weights")

    def dif_represent(self, X, table, lo, hi, net, first, count, W, w_off, R):
        """R float32 [count, rows, q]: the nets of the blocks first .. first + count - 1 (weights W at w_off) applied to the
        min-max scaled rows of X [rows, d] restricted to the features of the block's subspace."""
        _mat(X, "X"), _vec(lo, "lo"), _vec(hi, "hi"), _vec(W, "W"), _vec(w_off, "w_off", torch.int64), _vec(R, "R")
        feat, feat_off, _ = table
        rows, d = X.shape
        r, hidden, q, act = net
        assert lo.numel() == d and hi.numel() == d and w_off.numel() >= count and R.numel() >= count * rows * q
        assert (first + count - 1) // r < feat_off.numel() - 1
        harr = (ctypes.c_int32 * max(len(hidden), 1))(*hidden)
        _lib.check(self.lib.vgan_dif_represent(_ptr(X), X.stride(0), rows, d, _ptr(feat), _ptr(feat_off), _ptr(lo), _ptr(hi), int(r),
                                               int(first), int(count), len(hidden), harr, int(q), int(act), _ptr(W), _ptr(w_off),
                                               _ptr(R), self._stream()), "vgan_dif_represent")

    # ---- trained MLPs over subspaces (vgan_amd.outlier.SubspaceAutoEncoder / SubspaceDeepSVDD) ------------------------
    # net: (hidden tuple, activation code); state float32 with the block first + z at s_off[z] (int64 [count] on the device):
    # theta, m, v of P floats each, a layer K-major [K_l][N_l], with the autoencoder followed by its bias; scaling: (mean, scale)
    # float64 [d].  The two detectors' entries differ by the centre (float32 [count, q], q = hidden[-1]) that Deep SVDD's take
    # behind the Adam arguments (train) or the state (scores): center = () for an entry without one, else (tensor or None,).
    def _mlp_init(self, entry, layers, feat_off, net, first, count, scale, seed, state, s_off, total):
        """ae_init / svdd_init through the library's `entry`; `layers`: the layers of a net, so scale is float64 [S, layers]."""
        _vec(feat_off, "feat_off", torch.int32), _vec(scale, "scale", torch.float64), _vec(state, "state"), _vec(s_off, "s_off", torch.int64)
        hidden, _ = net
        assert state.numel() >= total and s_off.numel() >= count and first + count <= feat_off.numel() - 1
        assert scale.numel() >= (feat_off.numel() - 1) * layers
        harr = (ctypes.c_int32 * max(len(hidden), 1))(*hidden)
        _lib.check(getattr(self.lib, entry)(_ptr(feat_off), int(first), int(count), len(hidden), harr, _ptr(scale), int(seed), _ptr(state),
                                            _ptr(s_off), int(total), self._stream()), entry)

    def _mlp_train(self, entry, X, table, scaling, skip, net, first, count, max_dims, batch, seed, step_first, corr, adam, state, s_off, loss,
                   scratch, center=()):
        """ae_train / svdd_train through the library's `entry`; the centre goes behind the Adam arguments."""
        _mat(X, "X"), _vec(skip, "skip", torch.int32), _vec(corr, "corr", torch.float64), _vec(state, "state")
        _vec(s_off, "s_off", torch.int64), _mat(loss, "loss")
        feat, feat_off, _ = table
        mean, scale = scaling
        _vec(mean, "mean", torch.float64), _vec(scale, "scale", torch.float64)
        n, d = X.shape
        hidden, act = net
        steps = corr.shape[0]
        assert corr.dim() == 2 and corr.shape[1] == 2 and mean.numel() == d and scale.numel() == d
        assert first + count <= feat_off.numel() - 1 <= skip.numel() and s_off.numel() >= count and loss.shape[0] >= count
        for c in center:
            _vec(c, "center")
            assert c.numel() >= count * hidden[-1]
        if scratch is not None:
            _vec(scratch, "scratch")
        harr = (ctypes.c_int32 * max(len(hidden), 1))(*hidden)
        lr, beta1, beta2, eps, weight_decay = adam
        _lib.check(getattr(self.lib, entry)(_ptr(X), X.stride(0), n, d, _ptr(feat), _ptr(feat_off), _ptr(mean), _ptr(scale), _ptr(skip),
                                            int(first), int(count), int(max_dims), len(hidden), harr, int(act), int(batch), int(seed),
                                            int(step_first), int(steps), _ptr(corr), float(lr), float(beta1), float(beta2), float(eps),
                                            float(weight_decay), *map(_ptr, center), _ptr(state), _ptr(s_off), _ptr(loss),
                                            loss.stride(0) if count > 1 else loss.shape[1], _ptr(scratch),
                                            scratch.numel() if scratch is not None else 0, self._stream()), entry)

    def _mlp_scores(self, entry, X, table, scaling, skip, net, first, count, max_dims, state, s_off, score, raw, scratch, center=()):
        """ae_scores / svdd_scores through the library's `entry`; the centre goes behind s_off.  raw: None, or (name, buffer,
        width) for the raw output of one net instead of scores: float32 [rows, width]; width None where only the device knows
        it (d_s of the block), so the size is not checked here."""
        _mat(X, "X"), _vec(skip, "skip", torch.int32), _vec(state, "state"), _vec(s_off, "s_off", torch.int64)
        feat, feat_off, _ = table
        mean, scale = scaling
        _vec(mean, "mean", torch.float64), _vec(scale, "scale", torch.float64)
        rows, d = X.shape
        hidden, act = net
        assert mean.numel() == d and scale.numel() == d and first + count <= feat_off.numel() - 1 <= skip.numel() and s_off.numel() >= count
        ld_score = 0
        if raw is not None:
            raw_name, raw, raw_width = raw
            _vec(raw, raw_name)
            assert count == 1 and (raw_width is None or raw.numel() >= rows * raw_width)
        else:
            _mat(score, "score")
            assert score.shape[0] >= count and score.shape[1] >= rows
            for c in center:
                _vec(c, "center")
                assert c.numel() >= count * hidden[-1]
            ld_score = score.stride(0) if score.shape[0] > 1 else score.shape[1]
        if scratch is not None:
            _vec(scratch, "scratch")
        harr = (ctypes.c_int32 * max(len(hidden), 1))(*hidden)
        _lib.check(getattr(self.lib, entry)(_ptr(X), X.stride(0), rows, d, _ptr(feat), _ptr(feat_off), _ptr(mean), _ptr(scale), _ptr(skip),
                                            int(first), int(count), int(max_dims), len(hidden), harr, int(act), _ptr(state), _ptr(s_off),
                                            *map(_ptr, center), _ptr(score), int(ld_score), _ptr(raw), _ptr(scratch),
                                            scratch.numel() if scratch is not None else 0, self._stream()), entry)

    def ae_init(self, feat_off, net, first, count, scale, seed, state, s_off, total):
        """state float32 [>= total]: zeroed (the moments), then the Philox weights and biases of the blocks first .. first +
        count - 1; scale float64 [S, 2 L]: c_l = 1 / sqrt(K_l) per subspace."""
        self._mlp_init("vgan_ae_init", 2 * len(net[0]), feat_off, net, first, count, scale, seed, state, s_off, total)

    def ae_train(self, X, table, scaling, skip, net, first, count, max_dims, batch, seed, step_first, corr, adam, state, s_off, loss,
                 scratch=None):
        """Runs the global steps step_first .. step_first + len(corr) - 1 (0-based) of the blocks first .. first + count - 1 in
        place, one workgroup per block; corr float64 [steps, 2]: 1 - beta1^t and 1 - beta2^t of every step; adam: (lr, beta1,
        beta2, eps, weight_decay); loss float32 [count, >= step_first + steps]: column g receives the batch loss of step g."""
        self._mlp_train("vgan_ae_train", X, table, scaling, skip, net, first, count, max_dims, batch, seed, step_first, corr, adam, state, s_off,
                        loss, scratch)

    def ae_scores(self, X, table, scaling, skip, net, first, count, max_dims, state, s_off, score=None, recon=None, scratch=None):
        """score float32 [count, >= rows] (a view into the score matrix may be given): the reconstruction distances of the rows
        of X under the nets of the blocks first .. first + count - 1; with recon (float32 [rows, d_s], count 1) the raw output
        of the net instead."""
        self._mlp_scores("vgan_ae_scores", X, table, scaling, skip, net, first, count, max_dims, state, s_off, score,
                         None if recon is None else ("recon", recon, None), scratch)

    def svdd_init(self, feat_off, net, first, count, scale, seed, state, s_off, total):
        """state float32 [>= total]: zeroed (the moments), then the Philox weights of the blocks first .. first + count - 1;
        scale float64 [S, L]: c_l = 1 / sqrt(K_l) per subspace."""
        self._mlp_init("vgan_svdd_init", len(net[0]), feat_off, net, first, count, scale, seed, state, s_off, total)

    def svdd_center(self, X, table, scaling, skip, net, first, count, max_dims, state, s_off, tile_sums, run_sums, n_total, center_eps,
                    center, n_clamped, scratch=None):
        """Adds the output sums of the rows of X (a multiple of 32 rows in every call but the last), tile by tile, to run_sums
        float64 [count, q] (zeroed by the caller before the first call); n_total > 0 marks the last call, which writes center
        float32 [count, q] (mean, center_eps rule) and n_clamped int32 [count].  tile_sums: float64 workspace [>= count tiles q]."""
        _mat(X, "X"), _vec(skip, "skip", torch.int32), _vec(state, "state"), _vec(s_off, "s_off", torch.int64)
        _vec(tile_sums, "tile_sums", torch.float64), _vec(run_sums, "run_sums", torch.float64)
        _vec(center, "center"), _vec(n_clamped, "n_clamped", torch.int32)
        feat, feat_off, _ = table
        mean, scale = scaling
        _vec(mean, "mean", torch.float64), _vec(scale, "scale", torch.float64)
        rows, d = X.shape
        hidden, act = net
        q = hidden[-1]
        assert mean.numel() == d and scale.numel() == d and first + count <= feat_off.numel() - 1 <= skip.numel() and s_off.numel() >= count
        assert run_sums.numel() >= count * q and center.numel() >= count * q and n_clamped.numel() >= count
        if scratch is not None:
            _vec(scratch, "scratch")
        harr = (ctypes.c_int32 * max(len(hidden), 1))(*hidden)
        _lib.check(self.lib.vgan_svdd_center(_ptr(X), X.stride(0), rows, d, _ptr(feat), _ptr(feat_off), _ptr(mean), _ptr(scale), _ptr(skip),
                                             int(first), int(count), int(max_dims), len(hidden), harr, int(act), _ptr(state), _ptr(s_off),
                                             _ptr(tile_sums), tile_sums.numel(), _ptr(run_sums), int(n_total), float(center_eps),
                                             _ptr(center), _ptr(n_clamped), _ptr(scratch),
                                             scratch.numel() if scratch is not None else 0, self._stream()), "vgan_svdd_center")

    def svdd_train(self, X, table, scaling, skip, net, first, count, max_dims, batch, seed, step_first, corr, adam, center, state, s_off,
                   loss, scratch=None):
        """ae_train's arguments and center float32 [count, q]: the global steps step_first .. step_first + len(corr) - 1 of the
        one-class objective, in place; loss float32 [count, >= step_first + steps]."""
        self._mlp_train("vgan_svdd_train", X, table, scaling, skip, net, first, count, max_dims, batch, seed, step_first, corr, adam, state,
                        s_off, loss, scratch, (center,))

    def svdd_scores(self, X, table, scaling, skip, net, first, count, max_dims, state, s_off, center=None, score=None, embed=None,
                    scratch=None):
        """score float32 [count, >= rows] (a view into the score matrix may be given): the squared distances of the images of
        the rows of X from center [count, q]; with embed (float32 [rows, q], count 1) the raw output of the net instead."""
        self._mlp_scores("vgan_svdd_scores", X, table, scaling, skip, net, first, count, max_dims, state, s_off, score,
                         None if embed is None else ("embed", embed, net[0][-1]), scratch, (center,))

    # ---- iNNE over subspaces (vgan_amd.outlier.SubspaceINNE) -----------------------------------------------
    # state: (rows int32, r2 float64, nn int32, rho float64), each [S, T, psi]
    def inne_build(self, X, table, first, count, max_dims, ratio, seed, state):
        """state receives the T estimators of the subspaces first .. first + count - 1, built from X [n, d] on psi sampled
        rows each; max_dims: the most features of a subspace of the range; ratio: VGAN_INNE_RATIO_*."""
        rows, r2, nn, rho = state
        _mat(X, "X"), _vec(rows, "rows", torch.int32), _vec(nn, "nn", torch.int32)
        _vec(r2, "r2", torch.float64), _vec(rho, "rho", torch.float64)
        feat, feat_off, _ = table
        n, d = X.shape
        S, T, psi = rows.shape
        assert r2.shape == rows.shape and nn.shape == rows.shape and rho.shape == rows.shape and first + count <= S
        _lib.check(self.lib.vgan_inne_build(_ptr(X), X.stride(0), n, d, _ptr(feat), _ptr(feat_off), int(first), int(count), int(max_dims),
                                            T, psi, int(ratio), int(seed), _ptr(rows), _ptr(r2), _ptr(nn), _ptr(rho), self._stream()),
                   "vgan_inne_build")

    def inne_scores(self, Xq, X, table, first, count, max_dims, state, score):
        """score float32 [count, nq] (a view into the score matrix may be given): per query row of Xq and subspace of the
        range, the mean isolation score over the subspace's estimators; X [n, d]: the matrix they were built from."""
        rows, r2, _, rho = state
        _mat(Xq, "Xq"), _mat(X, "X"), _mat(score, "score")
        _vec(rows, "rows", torch.int32), _vec(r2, "r2", torch.float64), _vec(rho, "rho", torch.float64)
        feat, feat_off, _ = table
        nq, d = Xq.shape
        S, T, psi = rows.shape
        assert X.shape[1] == d and r2.shape == rows.shape and rho.shape == rows.shape and first + count <= S
        assert score.shape[0] == count and score.shape[1] >= nq
        _lib.check(self.lib.vgan_inne_scores(_ptr(Xq), Xq.stride(0), nq, d, _ptr(X), X.stride(0), X.shape[0], _ptr(feat), _ptr(feat_off),
                                             int(first), int(count), int(max_dims), T, psi, _ptr(rows), _ptr(r2), _ptr(rho), _ptr(score),
                                             score.stride(0), self._stream()), "vgan_inne_scores")

    # ---- Mahalanobis / MCD over subspaces (vgan_amd.outlier.SubspaceMahalanobis) ----------------------------
    # table: (feat int32, feat_off int32 [S + 1], sq_off int64 [S + 1]); the matrices of subspace s start at sq_off[s]
    def maha_moments(self, X, table, first, count, total_dims, max_dims, tiles, support, hcount, mean, cov, workspace):
        """mean (float64, at feat_off[s]) and cov (float64 [d_s, d_s] at sq_off[s]) of the subspaces first .. first + count - 1
        over the rows of X whose support byte is 1 (support uint8 [S, n]; None: every row); hcount int32 [S] their number;
        tiles int32 [n_tiles, 3]: the lower-triangle tiles (s, ti, tj) of the range; workspace: float64."""
        _mat(X, "X"), _vec(tiles, "tiles", torch.int32), _vec(hcount, "hcount", torch.int32)
        _vec(mean, "mean", torch.float64), _vec(cov, "cov", torch.float64), _vec(workspace, "workspace", torch.float64)
        feat, feat_off, sq_off = table
        n, d = X.shape
        if support is not None:
            _vec(support, "support", torch.uint8)
            assert support.dim() == 2 and support.shape[0] >= first + count and support.shape[1] == n
        assert tiles.dim() == 2 and tiles.shape[1] == 3 and hcount.numel() >= first + count
        _lib.check(self.lib.vgan_maha_moments(_ptr(X), X.stride(0), n, d, _ptr(feat), _ptr(feat_off), _ptr(sq_off), int(first), int(count),
                                              int(total_dims), int(max_dims), _ptr(tiles), tiles.shape[0], _ptr(support), n, _ptr(hcount),
                                              _ptr(mean), _ptr(cov), _ptr(workspace), workspace.numel() * 8, self._stream()),
                   "vgan_maha_moments")

    def maha_factor(self, cov, table, first, count, max_dims, hcount, shrinkage, L, W, alpha, status):
        """cov becomes the shrunk matrix (shrinkage in [0, 1], or -1 for OAS), L its lower Cholesky factor, W = L^-1; alpha
        float64 [S] the shrinkage used; status int32 [S]: bit 0 a constant subspace, bit 1 a failed pivot (sticky)."""
        for name, v in (("cov", cov), ("L", L), ("W", W), ("alpha", alpha)):
            _vec(v, name, torch.float64)
        _vec(hcount, "hcount", torch.int32), _vec(status, "status", torch.int32)
        _, feat_off, sq_off = table
        assert alpha.numel() >= first + count and status.numel() >= first + count and L.numel() >= cov.numel() <= W.numel()
        _lib.check(self.lib.vgan_maha_factor(_ptr(cov), _ptr(sq_off), _ptr(feat_off), int(first), int(count), int(max_dims), _ptr(hcount),
                                             float(shrinkage), _ptr(L), _ptr(W), _ptr(alpha), _ptr(status), self._stream()),
                   "vgan_maha_factor")

    def maha_scores(self, Xq, table, first, count, max_dims, mean, W, score):
        """score float32 [S, rows] (a view into the score matrix may be given): rows first .. first + count - 1 receive the
        squared Mahalanobis distances of the rows of Xq."""
        _mat(Xq, "Xq"), _mat(score, "score"), _vec(mean, "mean", torch.float64), _vec(W, "W", torch.float64)
        feat, feat_off, sq_off = table
        rows, d = Xq.shape
        assert score.shape[0] >= first + count and score.shape[1] >= rows
        _lib.check(self.lib.vgan_maha_scores(_ptr(Xq), Xq.stride(0), rows, d, _ptr(feat), _ptr(feat_off), _ptr(sq_off), int(first),
                                             int(count), int(max_dims), _ptr(mean), _ptr(W), _ptr(score), score.stride(0), self._stream()),
                   "vgan_maha_scores")

    def maha_select(self, score, first, count, hcount, support, changed):
        """support uint8 [S, n] = 1 on the hcount[s] rows with the smallest (score, row index); changed int32 [S]: whether
        that differs from what support held."""
        _mat(score, "score"), _vec(hcount, "hcount", torch.int32), _vec(support, "support", torch.uint8), _vec(changed, "changed", torch.int32)
        n = score.shape[1]
        assert support.dim() == 2 and support.shape[1] == n and min(score.shape[0], support.shape[0], changed.numel()) >= first + count
        _lib.check(self.lib.vgan_maha_select(_ptr(score), score.stride(0), n, int(first), int(count), _ptr(hcount), _ptr(support), n,
                                             _ptr(changed), self._stream()), "vgan_maha_select")

    # ---- PCA over subspaces (vgan_amd.outlier.SubspacePCA); table as for the Mahalanobis entries ----------------------
    def pca_eigen(self, cov, table, first, count, max_dims, standardize, max_sweeps, scale, evals, V, sweeps, status):
        """The eigenpairs of cov (or, with standardize, of the correlation matrix) of the subspaces first .. first + count - 1 by
        the fixed-order Jacobi sweeps: scale and evals (float64, at feat_off[s]; evals descending), V (float64 [d_s, d_s] at
        sq_off[s], row j the j-th component, signed), sweeps and status int32 [S] (bit 0 tr M == 0, bit 1 not converged).
        cov is overwritten."""
        for name, v in (("cov", cov), ("scale", scale), ("evals", evals), ("V", V)):
            _vec(v, name, torch.float64)
        _vec(sweeps, "sweeps", torch.int32), _vec(status, "status", torch.int32)
        _, feat_off, sq_off = table
        assert sweeps.numel() >= first + count and status.numel() >= first + count and V.numel() >= cov.numel()
        assert scale.numel() == evals.numel()
        _lib.check(self.lib.vgan_pca_eigen(_ptr(cov), _ptr(sq_off), _ptr(feat_off), int(first), int(count), int(max_dims),
                                           1 if standardize else 0, int(max_sweeps), _ptr(scale), _ptr(evals), _ptr(V), _ptr(sweeps),
                                           _ptr(status), self._stream()), "vgan_pca_eigen")

    def pca_scores(self, Xq, table, first, count, max_dims, mean, inv_scale, V, wt, score):
        """score float32 [S, rows] (a view into the score matrix may be given): rows first .. first + count - 1 receive sum_j wt_j
        y_j^2, y = V ((x - mean) inv_scale), of the rows of Xq; inv_scale and wt float64 at feat_off[s]."""
        _mat(Xq, "Xq"), _mat(score, "score")
        for name, v in (("mean", mean), ("inv_scale", inv_scale), ("V", V), ("wt", wt)):
            _vec(v, name, torch.float64)
        feat, feat_off, sq_off = table
        rows, d = Xq.shape
        assert score.shape[0] >= first + count and score.shape[1] >= rows and mean.numel() == inv_scale.numel() == wt.numel()
        _lib.check(self.lib.vgan_pca_scores(_ptr(Xq), Xq.stride(0), rows, d, _ptr(feat), _ptr(feat_off), _ptr(sq_off), int(first),
                                            int(count), int(max_dims), _ptr(mean), _ptr(inv_scale), _ptr(V), _ptr(wt), _ptr(score),
                                            score.stride(0), self._stream()), "vgan_pca_scores")

    # ---- Gaussian mixtures over subspaces (vgan_amd.outlier.SubspaceGMM) ------------------------------------
    # table: the EXPANDED table (feat int32, feat_off int32 [S C + 1], sq_off int64 [S C + 1]) of the entries e = s C + c;
    # first / count are subspaces; done int32 [S] or None
    def gmm_moments(self, X, table, n_components, first, count, total_dims, max_dims, tiles, resp, done, reg_covar, nk, weights,
                    log_weights, mean, cov, workspace):
        """nk, weights, log_weights (float64 [S C]), mean (at feat_off[e]) and cov (at sq_off[e]) of the subspaces first ..
        first + count - 1 that are not done, from X and the responsibilities resp (float64, count C n values); tiles int32
        [n_tiles, 3]: the lower-triangle tiles (e, ti, tj) of the range; total_dims: the sum of d_e over its entries."""
        _mat(X, "X"), _vec(tiles, "tiles", torch.int32), _vec(resp, "resp", torch.float64), _vec(workspace, "workspace", torch.float64)
        for name, v in (("nk", nk), ("weights", weights), ("log_weights", log_weights), ("mean", mean), ("cov", cov)):
            _vec(v, name, torch.float64)
        if done is not None:
            _vec(done, "done", torch.int32)
            assert done.numel() >= first + count
        feat, feat_off, sq_off = table
        n, d = X.shape
        entries = (first + count) * n_components
        assert tiles.dim() == 2 and tiles.shape[1] == 3 and resp.numel() >= count * n_components * n
        assert feat_off.numel() > entries and min(nk.numel(), weights.numel(), log_weights.numel()) >= entries
        _lib.check(self.lib.vgan_gmm_moments(_ptr(X), X.stride(0), n, d, _ptr(feat), _ptr(feat_off), _ptr(sq_off), int(n_components),
                                             int(first), int(count), int(total_dims), int(max_dims), _ptr(tiles), tiles.shape[0], _ptr(resp),
                                             _ptr(done), float(reg_covar), _ptr(nk), _ptr(weights), _ptr(log_weights), _ptr(mean),
                                             _ptr(cov), _ptr(workspace), workspace.numel() * 8, self._stream()), "vgan_gmm_moments")

    def gmm_logdet(self, L, table, n_components, first, count, logdet):
        """logdet float64 [S C]: sum_j log L_e[j, j] of the entries of the subspaces first .. first + count - 1."""
        _vec(L, "L", torch.float64), _vec(logdet, "logdet", torch.float64)
        _, feat_off, sq_off = table
        assert logdet.numel() >= (first + count) * n_components < feat_off.numel()
        _lib.check(self.lib.vgan_gmm_logdet(_ptr(L), _ptr(feat_off), _ptr(sq_off), int(n_components), int(first), int(count), _ptr(logdet),
                                            self._stream()), "vgan_gmm_logdet")

    def gmm_estep(self, Xq, table, n_components, first, count, max_dims, mean, W, logdet, log_weights, done=None, resp=None,
                  lb_partial=None, score=None):
        """The E step of the subspaces first .. first + count - 1 that are not done on the rows of Xq: resp (float64, count C
        rows values) the responsibilities, lb_partial (float64, count ceil(rows / 64) values) the sums of ln_i per 64 rows,
        score (float32 [S, rows], a view into the score matrix may be given) float32(-ln_i) in rows first .. of it."""
        _mat(Xq, "Xq")
        for name, v in (("mean", mean), ("W", W), ("logdet", logdet), ("log_weights", log_weights)):
            _vec(v, name, torch.float64)
        feat, feat_off, sq_off = table
        rows, d = Xq.shape
        assert feat_off.numel() > (first + count) * n_components <= min(logdet.numel(), log_weights.numel())
        if done is not None:
            _vec(done, "done", torch.int32)
            assert done.numel() >= first + count
        if resp is not None:
            _vec(resp, "resp", torch.float64)
            assert resp.numel() >= count * n_components * rows
        if lb_partial is not None:
            _vec(lb_partial, "lb_partial", torch.float64)
            assert lb_partial.numel() >= count * ((rows + 63) // 64)
        if score is not None:
            _mat(score, "score")
            assert score.shape[0] >= first + count and score.shape[1] >= rows
        _lib.check(self.lib.vgan_gmm_estep(_ptr(Xq), Xq.stride(0), rows, d, _ptr(feat), _ptr(feat_off), _ptr(sq_off), int(n_components),
                                           int(first), int(count), int(max_dims), _ptr(mean), _ptr(W), _ptr(logdet), _ptr(log_weights),
                                           _ptr(done), _ptr(resp), _ptr(lb_partial), _ptr(score),
                                           score.stride(0) if score is not None else 0, self._stream()), "vgan_gmm_estep")

    def gmm_converge(self, lb_partial, n, n_components, first, count, status, tol, iteration, done, n_iter, lower_bound, lb_prev):
        """sklearn's stop rule per subspace of the range, on the device: done / n_iter int32 [S], lower_bound / lb_prev float64
        [S]; status int32 [S C] is the factor's; iteration 0 only turns a failed status into a done flag."""
        _vec(status, "status", torch.int32), _vec(done, "done", torch.int32), _vec(n_iter, "n_iter", torch.int32)
        _vec(lower_bound, "lower_bound", torch.float64), _vec(lb_prev, "lb_prev", torch.float64)
        if lb_partial is not None:
            _vec(lb_partial, "lb_partial", torch.float64)
            assert lb_partial.numel() >= count * ((n + 63) // 64)
        assert status.numel() >= (first + count) * n_components
        assert min(done.numel(), n_iter.numel(), lower_bound.numel(), lb_prev.numel()) >= first + count
        _lib.check(self.lib.vgan_gmm_converge(_ptr(lb_partial), int(n), int(n_components), int(first), int(count), _ptr(status), float(tol),
                                              int(iteration), _ptr(done), _ptr(n_iter), _ptr(lower_bound), _ptr(lb_prev), self._stream()),
                   "vgan_gmm_converge")

    # ---- one-class SVM over subspaces (vgan_amd.outlier.SubspaceOCSVM) ---------------------------------------
    # K float32 [count, n, n], alpha / G float64 [count, n], done / n_iter int32 [count]: the arrays of one chunk.
    def ocsvm_kernel_matrix(self, P, sq, n, table, first, count, gamma, engine, splits, K):
        """K[z] = exp(-gamma[first + z] d2) of the packed block P against itself, the diagonal exactly 1."""
        _vec(P, "P"), _vec(gamma, "gamma", torch.float64), _vec(K, "K")
        assert K.numel() >= count * n * n and gamma.numel() >= first + count
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_ocsvm_kernel_matrix(_ptr(P), _ptr(sq), int(n), _ptr(feat_off), _ptr(col_off), int(first), int(count),
                                                     _ptr(gamma), int(engine), int(splits), _ptr(K), self._stream()),
                   "vgan_ocsvm_kernel_matrix")

    def _ocsvm_state(self, K, alpha, G, done, n_iter):
        _vec(K, "K"), _vec(alpha, "alpha", torch.float64), _vec(G, "G", torch.float64)
        _vec(done, "done", torch.int32), _vec(n_iter, "n_iter", torch.int32)
        if not (K.dim() == 3 and K.shape[1] == K.shape[2]):
            raise ValueError(f"K: need [count, n, n], got {tuple(K.shape)}")
        count, n = K.shape[0], K.shape[1]
        assert alpha.shape == (count, n) and G.shape == (count, n) and done.numel() >= count and n_iter.numel() >= count
        return count, n

    def ocsvm_init(self, K, m, a_m, alpha, G, done, n_iter):
        """libsvm's start: alpha = (1 x m, a_m, 0 ...), G = K alpha row after row, done = n_iter = 0."""
        count, n = self._ocsvm_state(K, alpha, G, done, n_iter)
        _lib.check(self.lib.vgan_ocsvm_init(_ptr(K), n, count, int(m), float(a_m), _ptr(alpha), _ptr(G), _ptr(done), _ptr(n_iter),
                                            self._stream()), "vgan_ocsvm_init")

    def ocsvm_smo(self, K, tol, max_iter, iterations, alpha, G, done, n_iter, storage=0):
        """Enqueues at most `iterations` SMO steps for every subspace of the chunk that is not done; reads nothing back."""
        count, n = self._ocsvm_state(K, alpha, G, done, n_iter)
        _lib.check(self.lib.vgan_ocsvm_smo(_ptr(K), n, count, float(tol), int(max_iter), int(iterations), int(storage), _ptr(alpha),
                                           _ptr(G), _ptr(done), _ptr(n_iter), self._stream()), "vgan_ocsvm_smo")

    def ocsvm_rho(self, alpha, G, rho):
        _vec(alpha, "alpha", torch.float64), _vec(G, "G", torch.float64), _vec(rho, "rho", torch.float64)
        count, n = alpha.shape
        assert G.shape == (count, n) and rho.numel() >= count
        _lib.check(self.lib.vgan_ocsvm_rho(_ptr(alpha), _ptr(G), n, count, _ptr(rho), self._stream()), "vgan_ocsvm_rho")

    def ocsvm_scores(self, Pq, sq_q, nq, Pr, sq_r, nr, table, first, count, gamma, alpha, rho, engine, splits, acc, score,
                     score_row=None):
        """score rows score_row = rho - sum_r alpha_r K(x_r, q) for the chunk; gamma / rho [S] and alpha [S, nr] are indexed by
        first + z."""
        _vec(gamma, "gamma", torch.float64), _vec(alpha, "alpha", torch.float64), _vec(rho, "rho", torch.float64)
        _vec(acc, "acc", torch.int64), _mat(score, "score")
        assert acc.numel() >= count * nq and alpha.shape[1] == nr and alpha.shape[0] >= first + count
        assert gamma.numel() >= first + count and rho.numel() >= first + count
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_ocsvm_scores(_ptr(Pq), _ptr(sq_q), int(nq), _ptr(Pr), _ptr(sq_r), int(nr), _ptr(feat_off), _ptr(col_off),
                                              int(first), int(count), _ptr(gamma), _ptr(alpha), _ptr(rho), int(engine), int(splits),
                                              _ptr(acc), _ptr(score), _ptr(score_row), score.stride(0), self._stream()),
                   "vgan_ocsvm_scores")

    # ---- kernel PCA over subspaces (vgan_amd.outlier.SubspaceKPCA) --------------------------------------------
    # K float32 [count, m, m] and R float32 [count, rows, m] are the arrays of one chunk; col_mean / wt float64 [S, m], total
    # float64 [S] and V float64 [S, m, m] are the fitted state of every subspace, indexed by first + z.
    def kpca_center(self, K, col_mean, total, Kc):
        """col_mean [count, m], total [count] and the centred matrices Kc float64 [count, m, m] (vgan_pca_eigen's input with the
        synthetic tables) from the upper triangles of K."""
        _vec(K, "K"), _vec(col_mean, "col_mean", torch.float64), _vec(total, "total", torch.float64), _vec(Kc, "Kc", torch.float64)
        if not (K.dim() == 3 and K.shape[1] == K.shape[2]):
            raise ValueError(f"K: need [count, m, m], got {tuple(K.shape)}")
        count, m = K.shape[0], K.shape[1]
        assert col_mean.numel() >= count * m and total.numel() >= count and Kc.numel() >= count * m * m
        _lib.check(self.lib.vgan_kpca_center(_ptr(K), m, count, _ptr(col_mean), _ptr(total), _ptr(Kc), self._stream()),
                   "vgan_kpca_center")

    def kpca_kernel_rows(self, Pq, sq_q, nq, Pr, sq_r, m, table, first, count, gamma, engine, splits, R):
        """R[z][q][c] = exp(-gamma[first + z] d2) of query row q of Pq and landmark row c of Pr, no diagonal rule."""
        _vec(Pq, "Pq"), _vec(Pr, "Pr"), _vec(gamma, "gamma", torch.float64), _vec(R, "R")
        assert R.numel() >= count * nq * m and gamma.numel() >= first + count
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_kpca_kernel_rows(_ptr(Pq), _ptr(sq_q), int(nq), _ptr(Pr), _ptr(sq_r), int(m), _ptr(feat_off),
                                                  _ptr(col_off), int(first), int(count), _ptr(gamma), int(engine), int(splits), _ptr(R),
                                                  self._stream()), "vgan_kpca_kernel_rows")

    def kpca_row_means(self, R, mean):
        """mean float64 [count, rows]: the mean of every row of R [count, rows, m] in the header's fixed order."""
        _vec(R, "R"), _vec(mean, "mean", torch.float64)
        count, rows, m = R.shape
        assert mean.numel() >= count * rows
        _lib.check(self.lib.vgan_kpca_row_means(_ptr(R), count * rows, m, _ptr(mean), self._stream()), "vgan_kpca_row_means")

    def kpca_scores(self, R, first, row_mean, col_mean, total, V, wt, score, score_row=None):
        """score rows score_row (or z), columns 0 .. rows - 1 = max(pot - proj, 0) of the rows of R [count, rows, m] (a view into
        the score matrix may be given)."""
        _vec(R, "R"), _mat(score, "score")
        for name, v in (("row_mean", row_mean), ("col_mean", col_mean), ("total", total), ("V", V), ("wt", wt)):
            _vec(v, name, torch.float64)
        count, rows, m = R.shape
        S = first + count
        assert row_mean.numel() >= count * rows and score.shape[1] >= rows
        assert col_mean.numel() >= S * m and wt.numel() >= S * m and total.numel() >= S and V.numel() >= S * m * m
        _lib.check(self.lib.vgan_kpca_scores(_ptr(R), rows, m, int(first), count, _ptr(row_mean), _ptr(col_mean), _ptr(total), _ptr(V),
                                             _ptr(wt), _ptr(score), _ptr(score_row), score.stride(0), self._stream()),
                   "vgan_kpca_scores")

    # ---- stochastic outlier selection over subspaces (vgan_amd.outlier.SubspaceSOS) --------------------------
    # D float32 [count, n, n] and beta / dmin / Z float64, n_iter / flags int32 [count, n]: the arrays of one chunk.
    def sos_distance_matrix(self, P, sq, n, table, first, count, metric, engine, splits, D):
        """D[z][c][q] = the dissimilarity (metric 0: sqrtf(d2), 1: d2) of rows q and c of the packed block P."""
        _vec(P, "P"), _vec(D, "D")
        assert D.numel() >= count * n * n
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_sos_distance_matrix(_ptr(P), _ptr(sq), int(n), _ptr(feat_off), _ptr(col_off), int(first), int(count),
                                                     int(metric), int(engine), int(splits), _ptr(D), self._stream()),
                   "vgan_sos_distance_matrix")

    def _sos_state(self, D, beta, dmin, Z):
        _vec(D, "D"), _vec(beta, "beta", torch.float64), _vec(dmin, "dmin", torch.float64), _vec(Z, "Z", torch.float64)
        if not (D.dim() == 3 and D.shape[1] == D.shape[2]):
            raise ValueError(f"D: need [count, n, n], got {tuple(D.shape)}")
        count, n = D.shape[0], D.shape[1]
        assert beta.shape == (count, n) and dmin.shape == (count, n) and Z.shape == (count, n)
        return count, n

    def sos_fit(self, D, perplexity, tol, max_iter, beta, dmin, Z, n_iter, flags, storage=0):
        """The perplexity search of every row of the chunk's matrices: beta, dmin, Z, the updates run and the flags (1: a
        degenerate row, 2: max_iter updates ran)."""
        count, n = self._sos_state(D, beta, dmin, Z)
        _vec(n_iter, "n_iter", torch.int32), _vec(flags, "flags", torch.int32)
        assert n_iter.shape == (count, n) and flags.shape == (count, n)
        _lib.check(self.lib.vgan_sos_fit(_ptr(D), n, count, float(perplexity), float(tol), int(max_iter), int(storage), _ptr(beta),
                                         _ptr(dmin), _ptr(Z), _ptr(n_iter), _ptr(flags), self._stream()), "vgan_sos_fit")

    def sos_fit_scores(self, D, beta, dmin, Z, score, score_row=None):
        """score rows score_row = the scores of the fitted rows themselves, from the chunk's stored matrices."""
        count, n = self._sos_state(D, beta, dmin, Z)
        _mat(score, "score")
        assert score.shape[1] >= n
        _lib.check(self.lib.vgan_sos_fit_scores(_ptr(D), n, count, _ptr(beta), _ptr(dmin), _ptr(Z), _ptr(score), _ptr(score_row),
                                                score.stride(0), self._stream()), "vgan_sos_fit_scores")

    def sos_scores(self, Pq, sq_q, nq, Pr, sq_r, nr, table, first, count, metric, beta, dmin, Z, engine, splits, acc, score,
                   score_row=None):
        """score rows score_row = the scores of the nq new rows for the chunk; beta / dmin / Z [S, nr] are indexed by first + z."""
        _vec(beta, "beta", torch.float64), _vec(dmin, "dmin", torch.float64), _vec(Z, "Z", torch.float64)
        _vec(acc, "acc", torch.int64), _mat(score, "score")
        assert acc.numel() >= count * nq and beta.shape[1] == nr and beta.shape[0] >= first + count
        assert dmin.shape == beta.shape and Z.shape == beta.shape
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_sos_scores(_ptr(Pq), _ptr(sq_q), int(nq), _ptr(Pr), _ptr(sq_r), int(nr), _ptr(feat_off), _ptr(col_off),
                                            int(first), int(count), int(metric), _ptr(beta), _ptr(dmin), _ptr(Z), int(engine),
                                            int(splits), _ptr(acc), _ptr(score), _ptr(score_row), score.stride(0), self._stream()),
                   "vgan_sos_scores")

    # ---- local correlation integral over subspaces (vgan_amd.outlier.SubspaceLOCI) ---------------------------
    # D float32 [count, n, n] (loci_distance_matrix), radii float32 [count, R], cnt / m int32 and S1 / S2 int64
    # [count, n, R]: the arrays of one chunk.
    def _loci_state(self, D, radii, *arrays):
        _vec(D, "D"), _vec(radii, "radii")
        if not (D.dim() == 3 and D.shape[1] == D.shape[2]):
            raise ValueError(f"D: need [count, n, n], got {tuple(D.shape)}")
        count, n, R = D.shape[0], D.shape[1], radii.shape[-1]
        assert radii.shape == (count, R)
        for t, name, dtype in arrays:
            _vec(t, name, dtype)
            assert t.shape == (count, n, R), (name, tuple(t.shape))
        return count, n, R

    def loci_distance_matrix(self, P, sq, n, table, first, count, engine, splits, D):
        """D[z][c][q] = sqrtf(d2) of rows q and c of the packed block P: sos_distance_matrix's Euclidean matrix, from 2 rows on."""
        _vec(P, "P"), _vec(D, "D")
        assert D.numel() >= count * n * n
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_loci_distance_matrix(_ptr(P), _ptr(sq), int(n), _ptr(feat_off), _ptr(col_off), int(first), int(count),
                                                      int(engine), int(splits), _ptr(D), self._stream()), "vgan_loci_distance_matrix")

    def loci_rmax(self, D, rmax):
        """rmax[z] = the largest off-diagonal entry of D[z]."""
        _vec(D, "D"), _vec(rmax, "rmax")
        if not (D.dim() == 3 and D.shape[1] == D.shape[2] and rmax.shape == (D.shape[0],)):
            raise ValueError(f"need D [count, n, n] and rmax [count], got {tuple(D.shape)} and {tuple(rmax.shape)}")
        _lib.check(self.lib.vgan_loci_rmax(_ptr(D), D.shape[1], D.shape[0], _ptr(rmax), self._stream()), "vgan_loci_rmax")

    def loci_counts(self, D, a, cnt):
        """cnt[z][q][j] = the number of rows c with D[z][c][q] <= a[z][j], the diagonal taken as 0."""
        count, n, R = self._loci_state(D, a, (cnt, "cnt", torch.int32))
        _lib.check(self.lib.vgan_loci_counts(_ptr(D), n, count, _ptr(a), R, _ptr(cnt), self._stream()), "vgan_loci_counts")

    def loci_sums(self, D, r, cnt, m, S1, S2):
        """Over the rows c with D[z][c][p] <= r[z][j]: m their number, S1 the sum of cnt[z][c][j], S2 that of its square."""
        count, n, R = self._loci_state(D, r, (cnt, "cnt", torch.int32), (m, "m", torch.int32), (S1, "S1", torch.int64),
                                       (S2, "S2", torch.int64))
        _lib.check(self.lib.vgan_loci_sums(_ptr(D), n, count, _ptr(r), R, _ptr(cnt), _ptr(m), _ptr(S1), _ptr(S2), self._stream()),
                   "vgan_loci_sums")

    def loci_finish(self, cnt, m, S1, S2, n_min, score, score_row=None, best=None):
        """score rows score_row = the largest valid num / sqrt(den) (or 0) of every row of the chunk; best int32, laid out as
        score: the lowest radius index that attains it, -1 where the score is 0."""
        _vec(cnt, "cnt", torch.int32), _vec(m, "m", torch.int32), _vec(S1, "S1", torch.int64), _vec(S2, "S2", torch.int64)
        count, n, R = cnt.shape
        assert m.shape == cnt.shape and S1.shape == cnt.shape and S2.shape == cnt.shape
        _mat(score, "score")
        assert score.shape[1] >= n
        if best is not None:
            _vec(best, "best", torch.int32)
            assert best.shape == score.shape and best.stride(0) == score.stride(0)
        _lib.check(self.lib.vgan_loci_finish(_ptr(cnt), _ptr(m), _ptr(S1), _ptr(S2), n, count, R, int(n_min), _ptr(score),
                                             _ptr(score_row), score.stride(0), _ptr(best), self._stream()), "vgan_loci_finish")

    def loci_scores(self, Pq, sq_q, nq, Pr, sq_r, nr, table, first, count, r, a, cnt, n_min, engine, splits, acc, score,
                    score_row=None, best=None, dist_out=None):
        """score rows score_row = the scores of the nq new rows for the chunk, each appended alone to the fitted set; r / a
        [S, R] and cnt [S, nr, R] are indexed by first + z; acc int64 [count, nq, 4, R] leaves with A, M, T1, T2; dist_out
        float32 [nq, nr] (count 1) the distances that were counted."""
        _vec(r, "r"), _vec(a, "a"), _vec(cnt, "cnt", torch.int32), _vec(acc, "acc", torch.int64), _mat(score, "score")
        R = r.shape[1]
        assert a.shape == r.shape and r.shape[0] >= first + count and cnt.shape == (r.shape[0], nr, R)
        assert acc.numel() >= count * nq * 4 * R and score.shape[1] >= nq
        if best is not None:
            _vec(best, "best", torch.int32)
            assert best.shape == score.shape and best.stride(0) == score.stride(0)
        if dist_out is not None:
            _vec(dist_out, "dist_out")
            assert count == 1 and dist_out.numel() >= nq * nr
        _, feat_off, col_off = table
        _lib.check(self.lib.vgan_loci_scores(_ptr(Pq), _ptr(sq_q), int(nq), _ptr(Pr), _ptr(sq_r), int(nr), _ptr(feat_off), _ptr(col_off),
                                             int(first), int(count), _ptr(r), _ptr(a), _ptr(cnt), int(R), int(n_min), int(engine),
                                             int(splits), _ptr(acc), _ptr(dist_out), _ptr(score), _ptr(score_row), score.stride(0),
                                             _ptr(best), self._stream()), "vgan_loci_scores")

    # ---- subspace outlier degree over subspaces (vgan_amd.outlier.SubspaceSOD) -------------------------------
    # Lists are int32 [count, rows, k]; the reverse lists of a chunk are rn_off int32 [count, n + 1], rn_rows int32 [count, n k].
    def sod_reverse_lists(self, idx, rn_off, rn_rows, cursor):
        """The reverse lists of the fit-time lists idx [count, n, k] as a CSR per subspace; cursor int32 [count, n] is scratch."""
        for t, name in ((idx, "idx"), (rn_off, "rn_off"), (rn_rows, "rn_rows"), (cursor, "cursor")):
            _vec(t, name, torch.int32)
        count, n, k = idx.shape
        assert rn_off.numel() >= count * (n + 1) and rn_rows.numel() >= count * n * k and cursor.numel() >= count * n
        _lib.check(self.lib.vgan_sod_reverse_lists(_ptr(idx), n, k, count, _ptr(rn_off), _ptr(rn_rows), _ptr(cursor), self._stream()),
                   "vgan_sod_reverse_lists")

    def sod_reference_sets(self, idxq, rn_off, rn_rows, nr, exclude_self, refset, n_unshared=None):
        """refset [count, nq, ref_set] = the first ref_set fitted rows by (shared neighbours descending, index ascending) of the
        lists idxq [count, nq, k] against the reverse lists; n_unshared [count] (fit) counts the sets that took a row sharing
        nothing."""
        for t, name in ((idxq, "idxq"), (rn_off, "rn_off"), (rn_rows, "rn_rows"), (refset, "refset")):
            _vec(t, name, torch.int32)
        count, nq, k = idxq.shape
        assert refset.dim() == 3 and refset.shape[:2] == (count, nq)
        assert rn_off.numel() >= count * (nr + 1) and rn_rows.numel() >= count * nr * k
        if n_unshared is not None:
            _vec(n_unshared, "n_unshared", torch.int32)
            assert n_unshared.numel() >= count
        _lib.check(self.lib.vgan_sod_reference_sets(_ptr(idxq), nq, _ptr(rn_off), _ptr(rn_rows), int(nr), k, count, refset.shape[2],
                                                    int(bool(exclude_self)), _ptr(refset), _ptr(n_unshared), self._stream()),
                   "vgan_sod_reference_sets")

    def sod_score(self, Xq, Xr, table, first, count, refset, alpha, form, score, score_row, n_relevant, mask=None):
        """SOD scores of the reference sets refset [count, nq, ref_set] into rows score_row of score, n_relevant int32 [count, nq];
        mask (int32 [count, nq, words], optional) receives the packed relevance bits over the positions of each subspace."""
        _mat(Xq, "Xq"), _mat(Xr, "Xr"), _vec(refset, "refset", torch.int32), _mat(score, "score")
        _vec(n_relevant, "n_relevant", torch.int32)
        feat, feat_off, _ = table
        nq = Xq.shape[0]
        assert Xq.shape[1] == Xr.shape[1] and refset.dim() == 3 and refset.shape[:2] == (count, nq)
        assert n_relevant.numel() >= count * nq and score.shape[1] >= nq
        words = 0
        if mask is not None:
            _vec(mask, "mask", torch.int32)
            assert mask.dim() == 3 and mask.shape[:2] == (count, nq)
            words = mask.shape[2]
        _lib.check(self.lib.vgan_sod_score(_ptr(Xq), Xq.stride(0), nq, _ptr(Xr), Xr.stride(0), Xr.shape[0], Xq.shape[1], _ptr(feat),
                                           _ptr(feat_off), int(first), int(count), _ptr(refset), refset.shape[2], float(alpha),
                                           int(form), _ptr(score), _ptr(score_row), score.stride(0), _ptr(n_relevant), _ptr(mask),
                                           int(words), self._stream()), "vgan_sod_score")


_default = None


def default_ops():
    global _default
    if _default is None:
        _default = HipOps()
    return _default

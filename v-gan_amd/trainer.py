"""Step engine of ``VGAN_no_kl.fit`` (reference: src/vgan.py:597-621) over a kernel provider.

One step = noise -> Generator_big (4 Linear) -> upper_softmax -> U*X -> MMDLossConstrained ->
backward -> Adadelta, launched as 11 asynchronous kernels (collapsed generator, bf16x3) on caller-owned, preallocated HBM
buffers and (on a GPU) replayed from one captured HIP graph per step.  Nothing in a step
synchronises the host: the loss is accumulated on the device and read once per epoch.

HBM layout (all float32 unless noted; n = global batch, nl = rows owned by this rank, d features,
dp = d rounded up to 4, L = latent size):
  flat params / grads / Adadelta state   one contiguous buffer each, parameter k at a 16-byte
                                          aligned offset, weights dense [out, in]
  data [Ntrain, d]                        whole training set, resident; batches are gathered by
                                          index inside the mask/projection kernel
  perm [batches_per_epoch, n] int32       this epoch's shuffled indices
  Z [2n, dp]  sq [2n]                     MMD operand [X_batch - c ; U*X_batch - c] (c = per-feature data mean) and its row norms
  Wg [nl, 2n]                             gradient weights of this rank's Y rows (never the 5x2nx2n K)
  S [nl, d], gU [slabs, nl, dp], dlogits  mask softmax, split-K slabs of dY*X, logits gradient

Generator (src/models/Generator.py:58-70 has NO activation between its Linear layers):
  "layered"    four GEMMs forward, seven backward, intermediate activations [nl, 2L..8L] kept;
  "collapsed"  (default) the chain in homogeneous coordinates: Wt_k = [[W_k, b_k],[0, 1]],
               At_k = Wt_k .. Wt_1, logits = [z|1] . At_4^T; backward from M4 = dlogits^T [z|1] ([d, L+1]):
               M_{k-1} = Wt_k^T M_k and dWt_k = M_k At_{k-1}^T.  Every product has an inner or outer dimension
               of L+1 instead of the batch: ~0.2 GFLOP/step instead of 2.5 at d=784, same mathematics
               (different fp32 association; parity-tested like the layered path).

Data parallel (exact): the O(n^2 d) work -- the Gram row block, the backward product -- and the mask
backward / weight-gradient contraction are sharded by rows: rank r owns rows [r*n/G, (r+1)*n/G) of the batch.  The
O(n d) front of the step (generator forward, mask, projection: ~10 us) is REPLICATED instead of exchanged: the data
set, the generator and the counter-based noise stream are replicated, so every rank can produce all n rows of U and Y
bit-identically, and with them the column arg-max keys.  That leaves ONE collective per step: all-reduce(SUM) of the
generator gradient (the flat gradient when layered; only M4, 10x smaller, when collapsed).  The loss is not needed by
the gradient: each rank accumulates its share of the block sums (rank 0 adds the penalty) and the shares are summed
once per epoch when the loss is read (`epoch_loss`, `step_loss`).  The bandwidth calibration of the first step is
replicated too.  Every rank applies the identical Adadelta update; results do not depend on G.
(An earlier version exchanged Y rows and a statistics record: three collectives per step, each ~a fifth of the
single-GPU step time at c3.)

Measured and rejected (MI355X, ROCm 7.2, c3): a fork/join HIP graph (XX tiles and weight-gradient GEMMs
on side streams) replays SLOWER than the plain chain (357 vs 313 us/step): each cross-stream edge costs
more than the overlap returns.  Re-measured on the final step with ONLY the X-X block sums (which feed the reported
loss, never a gradient) on a side stream that starts after the mask backward and joins at the end of the step:
161 vs 138 us/step, although dropping those tiles outright would save 7 us.

Which launches a step is made of is decided in step_plan.py (plan_step; the VGAN_* measurement knobs are listed on its Knobs
class); the engine below allocates for that plan and runs it.
"""
import contextlib
import gc
import os

import torch

from .step_plan import CHAIN_KPARTS_AUTO, Knobs, _best_boundary, _launch_rounds, _round4, chain_kparts, plan_step  # noqa: F401 (re-exported)

ADADELTA_RHO = 0.9   # torch.optim.Adadelta defaults used by the reference (src/vgan.py:567-568)
ADADELTA_EPS = 1e-6


@contextlib.contextmanager
def no_gc_while_capturing():
    """Around a HIP-graph capture.  Destroying a captured graph is not permitted while a stream captures, and torch terminates
    the process when it happens: an engine of an earlier fit that sits in a dead reference cycle is destroyed by whichever
    automatic garbage collection comes next, which may fall inside this capture (torch.cuda.graph no longer collects on
    entry).  So the dead cycles are collected BEFORE the capture begins, and the automatic collector rests until it ends."""
    was_enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


class FlatParams:
    """Re-homes a module's parameters into one flat buffer (16-byte aligned offsets) so that Adadelta
    and the gradient all-reduce are single streaming passes.  ``module`` keeps working: each
    parameter's ``.data`` becomes a view of the flat buffer."""

    def __init__(self, params, device):
        self.shapes = [tuple(p.shape) for p in params]
        self.offsets = []
        off = 0
        for p in params:
            self.offsets.append(off)
            off += _round4(p.numel())
        self.total = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros_like(self.flat)
        self.sq = torch.zeros_like(self.flat)
        self.acc = torch.zeros_like(self.flat)
        for k, (p, o) in enumerate(zip(params, self.offsets)):
            self.flat[o:o + p.numel()].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
            p.data = self.view(self.flat, k)

    def view(self, buf, k):
        o, shp = self.offsets[k], self.shapes[k]
        numel = 1
        for s in shp:
            numel *= s
        return buf[o:o + numel].view(shp)


class NoKLStepEngine:
    def __init__(self, ops, generator, data, batch_size, batches_per_epoch, lr=0.007, weight_decay=0.04, penalty_weight=10.0,
                 seed=777, noise="device", rank=0, world=1, group=None, use_graph=True, loss_accum_scale=None,
                 generator_mode=None, force_exchange=False, mmd_precision=None, center_operand=True, overlap_exchange=None,
                 fuse_update=None, front=None, chain_assoc=None):
        """Decides the step's schedule (step_plan.plan_step: every decision, its reasons and its measurements are there) and
        allocates the buffers that schedule needs."""
        self.ops = ops
        self.dev = data.device
        self.rank, self.world, self.group = rank, world, group
        n = self.n = int(batch_size)
        self.data = data
        d = self.d = data.shape[1]
        self.nb = int(batches_per_epoch)
        self.lr, self.wd, self.pen = float(lr), float(weight_decay), float(penalty_weight)
        self.seed = int(seed)
        self.noise_mode = noise
        self.use_graph = bool(use_graph) and data.is_cuda
        self.graph = None
        self.graph_multi = None          # `steps_per_graph` steps in one graph (run_steps)
        self.graph_blocks = {}           # block size -> captured graph (False: capture failed; the one-step graph keeps working)
        self.steps_per_graph = max(1, min(16, int(batches_per_epoch)))
        self.steps_done = 0
        self._xx_primed = False  # overlap mode: have the X-X sums of the upcoming batch been computed?
        self._coalesce = None    # sharded front: may the gathers share one collective launch?  (probed at first use)
        lin = [m for m in generator.main if isinstance(m, torch.nn.Linear)]
        assert len(lin) == 4
        L = self.L = lin[0].in_features
        self.widths = [L] + [m.out_features for m in lin]
        tables = {}  # host tile tables the plan counted: the chosen one is not built twice
        self.plan = plan_step(ops, n=n, d=d, data_stride=data.stride(0), latent=L, widths=self.widths, world=world, rank=rank,
                              force_exchange=force_exchange, generator_mode=generator_mode, mmd_precision=mmd_precision,
                              overlap_exchange=overlap_exchange, fuse_update=fuse_update, front=front, chain_assoc=chain_assoc,
                              knobs=Knobs.from_env(), host_tables=tables)
        vars(self).update(vars(self.plan))  # the step methods read the decisions as plain attributes: self.mode, self.bf3, ...
        self._alloc_generator([q for m in lin for q in (m.weight, m.bias)])
        self._alloc_mmd(center_operand)
        self.perm = torch.zeros(self.nb, n, dtype=torch.int32, device=self.dev)
        # the NEXT epoch's table, staged while the current epoch runs (stage_epoch_batches / begin_epoch)
        self.perm_next = torch.zeros_like(self.perm)
        self.epoch_staged = False
        self._alloc_carriers()
        self._alloc_tiles(tables[self.gram_tile, self.tile_split])
        self._hist, self._hist_n, self._hist_events = None, 0, []  # per-epoch mean losses kept on the device (close_epoch)
        self._read_stream, self._loss_host = None, None
        self.accum_scale = (1.0 / self.nb) if loss_accum_scale is None else float(loss_accum_scale)
        if self.front_sharded and data.is_cuda and self._collect().is_initialized():
            self._coalesce = self._probe_coalescing(self._collect())  # here, eagerly: the first exchange may run inside a capture

    def _alloc_generator(self, params):
        """Flat parameters, noise / logits of all batch rows, and the generator's chain (collapsed) or activations (layered)."""
        ops, n, nl, d, L, e = self.ops, self.n, self.nl, self.d, self.L, self.e
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.fp = FlatParams(params, self.dev)
        self.W = [self.fp.view(self.fp.flat, 2 * k) for k in range(4)]
        self.b = [self.fp.view(self.fp.flat, 2 * k + 1) for k in range(4)]
        self.za = torch.zeros(n, e[0], **f32)       # [z | 1 | 0-pad] for ALL batch rows (noise stream is replicated)
        self.za[:, L] = 1.0
        self.z_own = self.za[self.lo:self.lo + nl]
        self.logits = torch.zeros(n, d, **f32)      # all rows on every rank (replicated front, see the module docstring)
        self._chain = None  # logits job of the mask / projection launch (chain_in_mask), built at first use
        if self.mode == "layered":
            self.gslab = torch.zeros(self.splits, self.fp.total, **f32) if self.splits > 1 else None
            gbase = self.gslab[0] if self.splits > 1 else self.fp.grad
            self.dW = [self.fp.view(gbase, 2 * k) for k in range(4)]
            self.db = [self.fp.view(gbase, 2 * k + 1) for k in range(4)]
            self.acts = [self.za[:, :L]] + [torch.zeros(n, w, **f32) for w in self.widths[1:4]] + [self.logits]
            self.acts_own = [a[self.lo:self.lo + nl] for a in self.acts]
            self.dacts = [None] + [torch.zeros(nl, w, **f32) for w in self.widths[1:4]]
            return
        # packed weights Wt_k = [[W_k, b_k],[0, 1]] and packed gradients Gt_k = [dW_k | db_k] share ONE offset table, so
        # Adadelta can read the gradient of a flat element and write its updated value through a single index map
        poff = [0]
        for k in range(1, 5):
            poff.append(poff[-1] + e[k] * e[k - 1])
        self.Wt_all = torch.zeros(poff[-1], **f32)
        self.Gt_all = torch.zeros(poff[-1], **f32)
        self.Wt = [None] + [self.Wt_all[poff[k - 1]:poff[k]].view(e[k], e[k - 1]) for k in range(1, 5)]
        self.Gt = [None] + [self.Gt_all[poff[k - 1]:poff[k]].view(e[k], e[k - 1]) for k in range(1, 5)]
        self.At = [None, self.Wt[1]] + [torch.zeros(e[k], e[0], **f32) for k in range(2, 5)]  # Wt_k .. Wt_1 (At_1 = Wt_1)
        self.M = [None, self.Gt[1]] + [torch.zeros(e[k], e[0], **f32) for k in range(2, 5)]   # M_1 IS Gt_1 (At_0 = I)
        # suffix products B_3 = Wt_4 Wt_3 and B_2 = B_3 Wt_2: with them every M_k is one product away from M_4 and At_4 one
        # product away from At_2, so the chain is 3 + 2 dependent launches instead of 4 + 3 (each ~5 us whatever its size)
        self.B3 = torch.zeros(e[4], e[2], **f32)
        self.B2 = torch.zeros(e[4], e[1], **f32)
        self.At1s = torch.zeros(e[1], e[0], **f32)  # snapshot of Wt_1 for the launch that also updates it (fuse_update)
        if self.chain_flops:  # one workspace for the K-slice slabs of whichever product is running
            need = max([self.fwd_split[k] * e[k] * e[0] for k in (2, 3, 4)] + [self.bwd_split[k] * e[k - 1] * e[0] for k in (4, 3, 2)])
            self.chain_ws = torch.zeros(need, **f32)
        pmap = torch.full((self.fp.total,), -1, dtype=torch.int32)
        for k in range(1, 5):
            wk, wk1 = self.widths[k], self.widths[k - 1]
            r = torch.arange(wk, dtype=torch.int32)[:, None] * e[k - 1]
            ow, ob = self.fp.offsets[2 * (k - 1)], self.fp.offsets[2 * (k - 1) + 1]
            pmap[ow:ow + wk * wk1] = (poff[k - 1] + r + torch.arange(wk1, dtype=torch.int32)[None, :]).reshape(-1)
            pmap[ob:ob + wk] = (poff[k - 1] + r + wk1).reshape(-1)
        self.pmap = pmap.to(self.dev)
        self.pack_layers = [(self.W[k - 1], self.b[k - 1], self.Wt[k]) for k in range(1, 5)]
        self.unpack_layers = [(self.fp.view(self.fp.grad, 2 * (k - 1)), self.fp.view(self.fp.grad, 2 * (k - 1) + 1), self.Gt[k])
                              for k in range(1, 5)]
        ops.homogeneous_pack(self.pack_layers, unpack=False)  # once; afterwards Adadelta keeps Wt current

    def _alloc_mmd(self, center_operand):
        """The MMD operand [X - c ; U*X - c] with its norms and split images, the gradient weights and what the mask backward reads."""
        n, nl, d, dp = self.n, self.nl, self.d, self.dp
        f32, i16 = dict(dtype=torch.float32, device=self.dev), dict(dtype=torch.int16, device=self.dev)
        # The MMD operand is CENTRED: Z = [X - c ; U*X - c] with c = the per-feature mean of the data set (once per fit).
        # cdist(Z, Z)**2 and the backward expression sum_j W_ij (z_i - z_j) are translation invariant, so nothing changes in
        # exact arithmetic, but a feature's common offset mu no longer costs (mu/sigma)^2 of the operands' mantissa in
        # L = s_i + s_j - 2 g -- which decides the bf16x3 mode (16-bit operands) on unstandardised data.  Only `U * batch`'s
        # product rule needs the batch itself: the backward kernels add c back to their multiplier (`mul_shift`).
        self.center = torch.zeros(dp, **f32)
        if center_operand:
            self.ops.col_mean(self.data, self.center)
        self.S = torch.zeros(n, d, **f32)
        self.S_own = self.S[self.lo:self.lo + nl]
        self.Z = torch.zeros(2 * n, dp, **f32)
        self.sqn = torch.zeros(2 * n, **f32)   # bf16x3 mode: norms of the split values hi + lo (what its Gram multiplies)
        self.sq_cal = torch.zeros(2 * n, **f32) if self.bf3 else self.sqn  # fp32 norms for the (fp32) calibration launch
        self.Wg = torch.zeros(nl, 2 * n, **f32)
        self.gU_slabs = torch.zeros(self.bsplits, nl, dp, **f32)
        self.gU = self.gU_slabs[0]
        # [nl, d] view of a zero-padded [nl, dp] buffer: the M_4 product reads the padded matrix (vector loads for any d)
        self.dlogits_pad = torch.zeros(nl, dp, **f32)
        self.dlogits = self.dlogits_pad[:, :d]
        if self.bf3:
            self.Zh, self.Zl = torch.zeros(2 * n, self.kp, **i16), torch.zeros(2 * n, self.kp, **i16)
            if self.rm_backward:  # the backward reads the Gram's row-major images: no transposed copy of Z
                self.ZTh = self.ZTl = None
            else:
                self.ZTh, self.ZTl = torch.zeros(self.kp, self.kn, **i16), torch.zeros(self.kp, self.kn, **i16)
            self.Wh, self.Wl = torch.zeros(nl, self.kn, **i16), torch.zeros(nl, self.kn, **i16)

    def _alloc_tiles(self, host_table):
        """The Gram's tile table(s) -- `host_table`: the plan's, as ops.build_tiles returned it for plan.gram_tile and
        plan.tile_split --, the block sums they produce and the step tail's bookkeeping."""
        ops, n, nl, d, rank = self.ops, self.n, self.nl, self.d, self.rank
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.tiles = (host_table[0] if self.tile_split else host_table).to(self.dev)
        self.tiles_cal = self.tiles if self.cal_shares_tiles else ops.build_tiles(n, 0, 0, 1, device=self.dev)
        self.partial = torch.zeros(max(self.tiles.shape[0], self.tiles_cal.shape[0]), 4, **f32)
        self.stats = torch.zeros(4, dtype=torch.float64, device=self.dev)
        self.bw = torch.zeros(1, **f32)
        self.has_bw = False
        self.loss = torch.zeros(1, **f32)
        self.loss_accum = torch.zeros(1, **f32)
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.colpart = torch.zeros(self.col_chunks * d, dtype=torch.int64, device=self.dev)
        own = ops.colmax_chunks(nl) * d
        self.colpart_own = self.colpart[rank * own:(rank + 1) * own] if self.front_sharded else self.colpart
        self.colkey = torch.zeros(d, dtype=torch.int64, device=self.dev)
        self._fin = self._fold = None  # finalize jobs (raw pointers of the tensors above), built at first use

    def _alloc_carriers(self):
        """What only some schedules need: workspaces, the side stream, and the operands of work that rides in another launch."""
        ops, n, nl, dp, e = self.ops, self.n, self.nl, self.dp, self.e
        f32 = dict(dtype=torch.float32, device=self.dev)
        if self.two_stage_logits:
            self.T = torch.zeros(n, e[2], **f32)  # [z|1] . At_2^T
            self.T_ws = torch.zeros(((n + 63) // 64) * ((e[2] + 63) // 64) * 64 * _round4(e[1]), **f32)
        self.gram_tail_ws = ops.gram_tail_workspace(self.dev) if self.gram_tail else None
        self.rs_part = torch.zeros((2 * n + 127) // 128, nl, **f32) if self.rs_from_gram else None
        self._side = torch.cuda.Stream(device=self.dev) if (self.side_stream and self.data.is_cuda) else None
        self._xx = self._xx_m4 = self._rebuild = None  # jobs riding in another launch, built at first use
        if self.xx_ride:  # split images of the whole (centred) data set, prepared ONCE here
            i16 = dict(dtype=torch.int16, device=self.dev)
            rows_total = self.data.shape[0]
            self.Dh, self.Dl = torch.zeros(rows_total, self.kp, **i16), torch.zeros(rows_total, self.kp, **i16)
            self.dsq = torch.zeros(rows_total, **f32)
            ops.gather_rows_split(self.data, None, self.center, None, self.dsq, True, self.Dh, self.Dl, n=rows_total)
        # one zeroed workspace per K-split launch of the chain's backward, for the engine's life
        self.m4_ws = self.tn_ws = None
        if self.m4_kparts > 1:
            self.m4_ws = ops.ksplit_workspace(ops.linear_backward_params_ksplit_ws_bytes(e[0], dp, self.m4_kparts), self.dev)
        if self.tn_kparts > 1:
            tn = [("TN", self.Wt[4], self.M[4], self.M[3]), ("TN", self.B3, self.M[4], self.M[2]), ("TN", self.B2, self.M[4], self.M[1])]
            self.tn_ws = ops.ksplit_workspace(ops.gemm_grouped_ksplit_ws_bytes(tn, [self.tn_kparts] * 3), self.dev)
        self.xrow = torch.zeros(n, dtype=torch.int32, device=self.dev) if self.lean else None  # lean step: the batch's data-set rows

    # ---- host-side controls ---------------------------------------------------------------------
    def set_epoch_batches(self, idx):
        """idx: [batches_per_epoch, n] integer tensor of shuffled row indices (DataLoader order): the table of the epoch that
        starts now (= stage_epoch_batches + begin_epoch)."""
        if os.environ.get("VGAN_FEED_DIRECT") == "1":  # (A/B knob: the plain pageable copy of rounds 1-2)
            self.perm.copy_(idx.to(dtype=torch.int32), non_blocking=True)
            self._after_new_epoch_table()
            return
        self.stage_epoch_batches(idx)
        self.begin_epoch()

    def stage_epoch_batches(self, idx):
        """Host half of an epoch boundary, callable right after the previous epoch's steps have been launched: the table goes
        to a device staging buffer in stream order (behind those steps), so the host draw of the table (the DataLoader's
        randperm: ~90 us for 16 384 rows) overlaps the GPU's work instead of preceding the epoch's first launch."""
        self.perm_next.copy_(idx.to(dtype=torch.int32).view(self.nb, self.n), non_blocking=True)
        self.epoch_staged = True

    def begin_epoch(self):
        """Device half: the staged table becomes the current one (a 4 n nb byte device copy, same stream)."""
        if not self.epoch_staged:
            raise RuntimeError("begin_epoch without a staged table (stage_epoch_batches)")
        self.perm.copy_(self.perm_next)
        self.epoch_staged = False
        self._after_new_epoch_table()

    def _after_new_epoch_table(self):
        # overlap mode: the X-X sums of the batch the cursor points at were computed behind the previous step's all-reduce
        # from the OLD table; redo them for the new one (the first step of an epoch pays for them, the others do not)
        if self.overlap and self.has_bw:
            self._prefetch_xx()

    def _prefetch_xx(self):
        """X half of the operand of the batch the device-side cursor points at, and its X-X tiles (sums only)."""
        self._prefetch_x_operand()
        self._xx_tiles()
        self._xx_primed = True

    def _prefetch_x_operand(self):
        ops, n = self.ops, self.n
        rowsel = dict(row_cursor=self.step_counter, row_batches=self.nb, row_stride=n)
        if self.bf3:
            ops.gather_rows_split(self.data, self.perm, self.center, self.Z[:n], self.sqn[:n], True, self.Zh[:n], self.Zl[:n], **rowsel)
        else:
            ops.gather_rows_split(self.data, self.perm, self.center, self.Z[:n], self.sqn[:n], False, **rowsel)

    def _xx_tiles(self):
        ops, n = self.ops, self.n
        ntx = self.tiles.shape[0] - self.n_main
        if ntx == 0:
            return
        tx, px = self.tiles[self.n_main:], self.partial[self.n_main:self.n_main + ntx]
        if self.bf3:
            ops.mmd_gram_bf3(self.Zh, self.Zl, self.sqn, n, self.bw, tx, None, None, 0, px, tile=self.gram_tile)
        else:
            ops.mmd_gram(self.Z, self.sqn, n, self.dp, self.bw, tx, False, None, 0, px)

    def _fork_prefetch(self):
        """Starts the next step's parameter-independent work (`_prefetch_xx`) on the side stream."""
        if not self.overlap:
            return
        if self._side is None:  # CPU provider (tests) / "serial": same order of operations on one stream
            self._prefetch_xx()
            return
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            self._prefetch_xx()

    def _join_prefetch(self):
        if self.overlap and self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)

    def shuffle_epoch(self, epoch):
        """This epoch's shuffled drop_last batches from the device-side counter-based permutation (vgan_shuffle_epoch), keyed
        by (seed, epoch): identical on every rank, no host draw and no H2D copy."""
        self.ops.shuffle_epoch(self.perm, self.data.shape[0], self.seed, int(epoch))
        self._after_new_epoch_table()

    def set_bandwidth(self, value):
        self.bw.fill_(float(value))
        self.has_bw = True

    def set_noise(self, z):
        """Host-provided noise [n, L] for the next step (parity runs: the reference draws it on the CPU)."""
        self.za[:, :self.L].copy_(z.to(dtype=torch.float32), non_blocking=True)

    def epoch_loss(self):
        """Mean loss of the steps since the last call (one host sync), as the reference's
        ``generator_loss += loss / batch_number`` (src/vgan.py:620-621)."""
        v = float(self._sum_over_ranks(self.loss_accum).item())
        self.loss_accum.zero_()
        return v

    def close_epoch(self):
        """Device half of an epoch's loss read-out: the accumulated mean loss moves into the next slot of a device-side history
        (summed over the ranks when there are several) and the accumulator is cleared -- stream-ordered, no host sync.  Returns the
        slot; `read_epoch_loss(slot)` fetches it later, on a side stream, without waiting for work launched in between, so that
        a fit can report epoch e while the GPU already runs epoch e + 1."""
        if self._hist is None or self._hist_n == self._hist.numel():
            grown = torch.zeros(max(64, 2 * self._hist_n), dtype=torch.float32, device=self.dev)
            if self._hist is not None:
                grown[:self._hist_n].copy_(self._hist)
            self._hist = grown
        slot = self._hist_n
        cell = self._hist[slot:slot + 1]
        cell.copy_(self.loss_accum)
        self.loss_accum.zero_()
        if self.exchange:
            self._collect().all_reduce(cell, group=self.group)
        ev = None
        if self.data.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        self._hist_events.append(ev)
        self._hist_n += 1
        return slot

    def read_epoch_loss(self, slot):
        """Host half: the mean loss `close_epoch` stored in `slot` (waits for that epoch only)."""
        ev = self._hist_events[slot]
        if ev is None:
            return float(self._hist[slot])
        if self._read_stream is None:
            self._read_stream = torch.cuda.Stream(self.dev)
            self._loss_host = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._read_stream.wait_event(ev)
        with torch.cuda.stream(self._read_stream):
            self._loss_host.copy_(self._hist[slot:slot + 1], non_blocking=True)
        self._read_stream.synchronize()
        return float(self._loss_host[0])

    def step_loss(self):
        """Loss of the last step (one host sync; with several ranks also one tiny all-reduce: `loss` holds this rank's share)."""
        return float(self._sum_over_ranks(self.loss).item())

    def _sum_over_ranks(self, t):
        if not self.exchange:
            return t
        t = t.clone()
        self._collect().all_reduce(t, group=self.group)
        return t

    def grad_view(self, k):
        """Gradient of parameter tensor k as of the last step (sums split-K slabs that Adadelta consumed directly)."""
        if self.mode == "collapsed":
            self.ops.homogeneous_pack(self.unpack_layers, unpack=True)  # packed gradients -> flat layout (inspection only)
        elif not self.exchange and self.splits > 1:
            return sum(self.fp.view(self.gslab[sl], k) for sl in range(self.splits))
        return self.fp.view(self.fp.grad, k)

    # ---- generator -----------------------------------------------------------------------------------
    def _generator_forward(self, own_rows=False):
        """own_rows: logits of this rank's batch rows only (sharded front)."""
        ops = self.ops
        if self.mode == "layered":
            for k in range(4):
                ops.linear_forward(self.acts[k], self.W[k], self.b[k], self.acts[k + 1])
            return
        # prefix products At_k = Wt_k .. Wt_1 (Wt is kept current by the optimiser)
        Wt, At = self.Wt, self.At
        if self.chain_flops:  # flop-minimal association: every product is [e_k, e_{k-1}] x [e_{k-1}, e0]
            for k in (2, 3, 4):
                sp = self.fwd_split[k]
                if sp > 1:
                    ops.gemm_grouped([("NN", Wt[k], At[k - 1], self._slabs(sp, At[k]), sp)])
                    ops.reduce_slabs(self.chain_ws, At[k].numel(), sp, At[k])
                else:
                    ops.gemm_grouped([("NN", Wt[k], At[k - 1], At[k])])
        elif self.two_stage_logits:
            # ... and the logits WITHOUT a launch of their own: T = [z|1] . At_2^T = ([z|1] . Wt_1^T) . Wt_2^T rides in the first
            # level as a two-stage tile (vgan_gemm_problem NT_NT), logits = T . B_3^T in the second beside At_3 and B_2.  At_4 is
            # then not formed at all (nothing but the logits read it): forward 3 -> 2 dependent launches.
            ops.gemm_grouped([("NN", Wt[2], At[1], At[2]), ("NN", Wt[4], Wt[3], self.B3), ("NT2", self.za, Wt[1], self.T, Wt[2], self.T_ws)])
            ops.gemm_grouped([("NN", Wt[3], At[2], At[3]), ("NN", self.B3, Wt[2], self.B2), ("NT", self.T, self.B3[:self.d], self.logits)])
            return
        else:                 # two dependency levels through the suffix products B_3, B_2
            ops.gemm_grouped([("NN", Wt[2], At[1], At[2]), ("NN", Wt[4], Wt[3], self.B3)])
            ops.gemm_grouped([("NN", Wt[3], At[2], At[3]), ("NN", self.B3, At[2], At[4]), ("NN", self.B3, Wt[2], self.B2)])
        if own_rows:
            ops.linear_forward(self.z_own, At[4][:self.d], None, self.logits[self.lo:self.lo + self.nl])
        elif not self.chain_in_mask:  # otherwise logits = [z|1] . At_4^T are formed inside the mask / projection launch
            ops.linear_forward(self.za, At[4][:self.d], None, self.logits)

    def _slabs(self, splits, like):
        """[splits, rows, cols] view of the chain workspace for the K-slice partial products of a matrix shaped like `like`."""
        return self.chain_ws[:splits * like.numel()].view(splits, like.shape[0], like.shape[1])

    def _generator_backward_update(self, dist):
        """dlogits -> parameter gradients -> (all-reduce) -> Adadelta."""
        ops = self.ops
        adadelta = dict(lr=self.lr, rho=ADADELTA_RHO, eps=ADADELTA_EPS, weight_decay=self.wd, grad_scale=1.0)
        if self.mode == "layered":
            g = self.dlogits
            for k in (3, 2, 1, 0):
                ops.linear_backward_params(g, self.acts_own[k], self.dW[k], self.db[k], self.splits, self.fp.total)
                if k:
                    ops.linear_backward_input(g, self.W[k], self.dacts[k])
                    g = self.dacts[k]
            if dist:
                if self.splits > 1:
                    ops.reduce_slabs(self.gslab, self.fp.total, self.splits, self.fp.grad)
                dist.all_reduce(self.fp.grad, group=self.group)
                ops.adadelta_step(self.fp.flat, self.fp.grad, self.fp.sq, self.fp.acc, **adadelta)
            elif self.splits > 1:  # no exchange: Adadelta sums the slabs itself
                ops.adadelta_step(self.fp.flat, self.gslab[0], self.fp.sq, self.fp.acc, nslabs=self.splits, slab_stride=self.fp.total,
                                  **adadelta)
            else:
                ops.adadelta_step(self.fp.flat, self.fp.grad, self.fp.sq, self.fp.acc, **adadelta)
            return
        e, d = self.e, self.d
        # M4[:d] = dlogits^T . [z|1]   (rows >= d stay zero: the homogeneous output coordinate carries no gradient)
        # (the library runs this long contraction on its tall-skinny 16-wave tiles.  Cutting it over more workgroups pays only
        # with the combine INSIDE the launch (m4_kparts, chain_kparts above): row slabs + a reduction launch, or slab-summing
        # staging loads in the consumers, were both measured slower)
        if self.xx_in_m4 and not self.xx_late_in_backward:
            ops.linear_backward_params_xx(self.dlogits_pad, self.z_own, self.M[4][:self.dp], self._late_xx_job())
        elif self.m4_kparts > 1:
            ops.linear_backward_params_ksplit(self.dlogits_pad, self.z_own, self.M[4][:self.dp], self.m4_kparts, self.m4_ws)
        else:
            ops.linear_backward_params(self.dlogits_pad, self.z_own, self.M[4][:self.dp], None)  # pad columns are zero: rows d.. of M_4 too
        if dist:
            dist.all_reduce(self.M[4], group=self.group)  # (the side stream's prefetch may still be running beside it)
        # M_{k-1} = Wt_k^T M_k, i.e. M_3 = Wt_4^T M_4, M_2 = B_3^T M_4, M_1 = B_2^T M_4 (At_0 = I: Gt_1 IS M_1), and
        # [dW_k | db_k] = Gt_k = M_k . At_{k-1}^T: two dependency levels
        M, Gt, At = self.M, self.Gt, self.At
        # (launches are kept homogeneous -- long contractions in one, short ones in the other -- so that the library can run
        # the long-K group on its 16-wave tiles)
        fused_noise = dict(next_noise=self.za, noise_cols=self.L, noise_ones_col=self.L, seed=self.seed,
                           step_counter=self.step_counter) if self.noise_mode == "device" else {}
        if self.chain_flops:
            # M_{k-1} = Wt_k^T M_k one after the other, each Gt_k = M_k At_{k-1}^T sharing a launch with the next M
            Wt = self.Wt
            for k in (4, 3, 2):
                sp = self.bwd_split[k]
                probs = [("TN", Wt[k], M[k], self._slabs(sp, M[k - 1]), sp) if sp > 1 else ("TN", Wt[k], M[k], M[k - 1])]
                if k < 4:
                    probs.append(("NT", M[k + 1], At[k], Gt[k + 1]))
                ops.gemm_grouped(probs, fold=self._fold if (self.xx_in_m4 and k == 4) else None)
                if sp > 1:
                    ops.reduce_slabs(self.chain_ws, M[k - 1].numel(), sp, M[k - 1])
            ops.gemm_grouped([("NT", M[2], At[1], Gt[2])])
            ops.adadelta_step_packed(self.fp.flat, self.pmap, self.Gt_all, self.Wt_all, self.fp.sq, self.fp.acc, **adadelta, **fused_noise)
            return
        tn_split = dict(kparts=[self.tn_kparts] * 3, ksplit_ws=self.tn_ws) if self.tn_kparts > 1 else {}
        if not self.fuse_update:
            ops.gemm_grouped([("TN", self.Wt[4], M[4], M[3]), ("TN", self.B3, M[4], M[2]), ("TN", self.B2, M[4], M[1])],
                             fold=self._fold if self.xx_in_m4 else None, **tn_split)
            ops.gemm_grouped([("NT", M[4], At[3], Gt[4]), ("NT", M[3], At[2], Gt[3]), ("NT", M[2], At[1], Gt[2])])
            ops.adadelta_step_packed(self.fp.flat, self.pmap, self.Gt_all, self.Wt_all, self.fp.sq, self.fp.acc, **adadelta, **fused_noise)
            return
        # The optimiser rides in the LAST product launch of the step: Gt_4, Gt_3, Gt_2 are updated in the epilogue of the tile
        # that produces them (flat parameter, Adadelta state and packed weight Wt_k in place), Gt_1 = M_1 (complete after the
        # launch before) by surplus workgroups, and the next step's noise draw rides along too -- no separate optimiser
        # launch.  Wt_1 is also an OPERAND of that launch (At_1 = Wt_1 in Gt_2 = M_2 . At_1^T), so the launch before it
        # snapshots it (a copy job riding there) and the product reads the snapshot.
        ops.gemm_grouped([("TN", self.Wt[4], M[4], M[3]), ("TN", self.B3, M[4], M[2]), ("TN", self.B2, M[4], M[1])],
                         copy=(self.Wt[1], self.At1s), fold=self._fold if self.xx_in_m4 else None, **tn_split)
        w, off = self.widths, self.fp.offsets
        layers = [(self.Wt[k], off[2 * (k - 1)], off[2 * (k - 1) + 1], w[k], w[k - 1]) for k in (4, 3, 2, 1)]
        ops.gemm_grouped([("NT", M[4], At[3], Gt[4]), ("NT", M[3], At[2], Gt[3]), ("NT", M[2], self.At1s, Gt[2])],
                         adadelta=dict(p=self.fp.flat, sq=self.fp.sq, acc=self.fp.acc, layers=layers, extra_grad=Gt[1], **adadelta),
                         noise=fused_noise or None)

    # ---- the step -----------------------------------------------------------------------------------
    def _collect(self):
        import torch.distributed as dist
        return dist

    def _forward(self):
        ops, n, nl, lo = self.ops, self.n, self.nl, self.lo
        if self.noise_mode == "device" and (self.mode == "layered" or self.steps_done == 0):
            # collapsed mode: every later draw rides in the previous step's optimiser launch (same Philox stream)
            ops.noise_normal(self.za, self.seed, self.step_counter, 0, cols=self.L, ones_col=self.L)
        self._generator_forward()
        rowsel = dict(row_cursor=self.step_counter, row_batches=self.nb, row_stride=n)
        logits = self.logits
        if self.chain_in_mask:
            if self._chain is None:
                self._chain = ops.logits_chain(self.za, self.At[4][:self.d])
            rowsel["chain"] = self._chain
            logits = None
        if self.fused_prepare:  # mask/projection and the bf16x3 operand split in one launch
            xx = None
            if self.xx_ride and self.has_bw:  # (before the bandwidth exists the first step runs these tiles after its calibration)
                if self._xx is None:
                    ntx = self.tiles.shape[0] - self.n_main
                    self._xx = ops.xx_job(self.Dh, self.Dl, self.dsq, self.tiles[self.n_main:], self.bw, self.partial[self.n_main:self.n_main + ntx])
                xx = self._xx
            if self.lean:  # (Z is written while the bandwidth does not exist: the calibration reads it)
                ops.mask_project_forward_bf3(logits, self.data, self.perm, self.S, self.Z, self.sqn, self.Zh, self.Zl, None, None,
                                             center=self.center, xx=xx, write_z=not self.has_bw, xrow=self.xrow, **rowsel)
            else:
                ops.mask_project_forward_bf3(logits, self.data, self.perm, self.S, self.Z, self.sqn, self.Zh, self.Zl, self.ZTh, self.ZTl,
                                             center=self.center, write_x=not self.x_ahead, xx=xx, **rowsel)
            return
        if self.x_ahead:  # the X half of Z / sq (and of the split images) is already in place
            ops.mask_project_forward(logits, self.data, self.perm, self.S, None, None, self.Z[n:], None, self.sqn[n:],
                                     row_offset=0, center=self.center, norm_split=self.bf3, **rowsel)
        else:
            ops.mask_project_forward(logits, self.data, self.perm, self.S, None, self.Z[:n], self.Z[n:], self.sqn[:n], self.sqn[n:],
                                     row_offset=0, center=self.center, norm_split=self.bf3, **rowsel)

    def _calibrate(self):
        """First-call bandwidth (src/models/Mmd_loss_constrained.py:16-20): sum(L) / (N^2 - N)."""
        ops = self.ops
        if self.bf3:  # sqn holds the norms of the split values; the calibration launch is the fp32 kernel on Z itself
            ops.row_sqnorm(self.Z, self.sq_cal, self.dp)
        ops.mmd_gram(self.Z, self.sq_cal, self.n, self.dp, None, self.tiles_cal, True, None, 0, self.partial)
        ops.mmd_reduce(self.partial, self.tiles_cal, self.stats, True)
        ops.mmd_set_bandwidth(self.stats, self.n, self.bw)
        self.has_bw = True

    def _loss_backward_update(self):
        ops, n, nl, lo, d = self.ops, self.n, self.nl, self.lo, self.d
        dist = self._collect() if self.exchange else None
        gstride = nl * self.dp
        if self.bf3 and not self.fused_prepare:
            if self.x_ahead:
                ops.mmd_bf3_prepare(self.Z[n:], n, d, self.Zh[n:], self.Zl[n:])
            else:
                ops.mmd_bf3_prepare(self.Z, 2 * n, d, self.Zh, self.Zl, self.ZTh, self.ZTl)
        if self.bf3:
            ops.mmd_gram_bf3(self.Zh, self.Zl, self.sqn, n, self.bw, self.tiles[:self.n_main], self.Wh, self.Wl, n + lo, self.partial, self.S, 0,
                             self.colpart, True, tile=self.gram_tile, tail_ws=self.gram_tail_ws, rs_part=self.rs_part)
        else:
            ops.mmd_gram_colmax(self.Z, self.sqn, n, self.dp, self.bw, self.tiles[:self.n_main], self.Wg, n + lo, self.partial, self.S, 0,
                                self.colpart, True)
        # the step tail (block sums -> stats, column keys, loss bookkeeping) rides in the backward launch as one extra
        # workgroup: its outputs are first needed by the mask backward, so it leaves the critical path.  With several
        # ranks `stats` / `loss` are this rank's share (its tiles); the penalty is added by rank 0 only.
        if self._fin is None:
            fin_args = (self.partial, self.tiles, self.colpart, ops.colmax_chunks(n), self.colkey, n, d, self.pen if self.rank == 0 else 0.0,
                        self.stats, self.loss, self.loss_accum, self.accum_scale, self.step_counter)
            if self.xx_in_m4:  # part of the X-X block sum arrives later in the step: the tail is split (include/vgan_hip.h)
                self._fin = ops.finalize_job(*fin_args, mode=1, ntiles_main=self.n_main)
                self._fold = ops.finalize_job(*fin_args, mode=2, ntiles_main=self.n_main)
            else:
                self._fin = ops.finalize_job(*fin_args)
        fin = self._fin
        if self.bf3:
            if self.lean:
                if self._rebuild is None:
                    self._rebuild = ops.bwd_rebuild(self.data, self.xrow, self.S, self.center)
                ops.mmd_backward_bf3_rm_rebuild(self.Wh, self.Wl, self.Zh, self.Zl, 2 * n, nl, d, self._rebuild, self.gU, self.bsplits, gstride,
                                                fin, xx=self._late_xx_job() if self.xx_late_in_backward else None)
            elif self.rm_backward:
                ops.mmd_backward_bf3_rm(self.Wh, self.Wl, self.Zh, self.Zl, 2 * n, self.Z, n + lo, nl, d, self.Z[lo:lo + nl], self.gU,
                                        self.bsplits, gstride, fin, mul_shift=self.center, tile=self.bwd_tile,
                                        xx=self._late_xx_job() if self.xx_late_in_backward else None, rs_part=self.rs_part)
            else:
                ops.mmd_backward_bf3(self.Wh, self.Wl, self.ZTh, self.ZTl, self.Z, n + lo, nl, d, self.Z[lo:lo + nl], self.gU, self.bsplits,
                                     gstride, fin, mul_shift=self.center, tile=self.bwd_tile)
        else:
            ops.mmd_backward(self.Wg, self.Z, n + lo, nl, 2 * n, self.dp, self.Z[lo:lo + nl], self.gU, self.bsplits, gstride, fin,
                             mul_shift=self.center)
        self._fork_prefetch()  # the batch cursor has advanced (step tail in the launch above); nothing below touches the X half
        ops.mask_backward(self.gU, self.S_own, self.colkey, self.pen, lo, self.dlogits, self.bsplits, gstride)
        self._generator_backward_update(dist)
        self._join_prefetch()

    # ---- sharded front ------------------------------------------------------------------
    def _forward_sharded(self):
        """Front of the step for this rank's n/G rows: logits, mask / projection, operand split, column keys."""
        ops, n, nl, lo, d = self.ops, self.n, self.nl, self.lo, self.d
        if self.noise_mode == "device" and self.steps_done == 0:
            ops.noise_normal(self.za, self.seed, self.step_counter, 0, cols=self.L, ones_col=self.L)
        self._generator_forward(own_rows=True)
        rowsel = dict(row_cursor=self.step_counter, row_batches=self.nb, row_stride=n)
        own, yown = slice(lo, lo + nl), slice(n + lo, n + lo + nl)
        # X half of the operand, ALL batch rows (every rank's XY tiles read all X columns; no parameter enters, so it is
        # gathered from the resident data set instead of exchanged): centred rows + norms (+ split images)
        if self.bf3:
            ops.gather_rows_split(self.data, self.perm, self.center, None, self.sqn[:n], True, self.Zh[:n], self.Zl[:n], **rowsel)
        else:
            ops.gather_rows_split(self.data, self.perm, self.center, self.Z[:n], self.sqn[:n], False, **rowsel)
        # (bf16x3: the backward's multiplier is the fp32 X row of an own row -- written here; fp32 mode has it from the gather)
        ops.mask_project_forward(self.logits[own], self.data, self.perm, self.S_own, None, self.Z[own] if self.bf3 else None, self.Z[yown],
                                 None, self.sqn[yown], row_offset=lo, center=self.center, norm_split=self.bf3, **rowsel)
        if self.bf3:
            ops.mmd_bf3_prepare(self.Z[yown], nl, d, self.Zh[yown], self.Zl[yown])
        ops.colmax_partial(self.S_own, lo, self.colpart_own)

    def _all_gather(self, dist, out, own):
        """all-gather of `own` (this rank's slice OF `out`, in place).  A process group smaller than the engine's world is the
        one-GPU shard emulation of tools/dp_selftest.py: the collective is issued on the slice alone."""
        size = dist.get_world_size(self.group) if dist.is_initialized() else 1
        if size != self.world:
            out = own
        if own.is_cuda and dist.get_backend(self.group) == "gloo":
            # rehearsal of several ranks on ONE GPU (tests/test_dp_gpu.py, bench.py with VGAN_BENCH_BACKEND=gloo): through the host
            host = out.cpu()
            dist.all_gather_into_tensor(host, own.cpu(), group=self.group)
            out.copy_(host)
            return None
        return dist.all_gather_into_tensor(out, own, group=self.group, async_op=True)

    def _exchange_front(self, dist):
        """The ONE exchange of the sharded front: Y rows of the operand (+ norms) and the column keys, all-gathered in place.
        Returns the pending work handles; the caller runs the tiles that need none of it meanwhile."""
        n, nl, lo = self.n, self.nl, self.lo
        yown = slice(n + lo, n + lo + nl)
        pairs = []
        if self.bf3:  # (int16 images travel as int32 words: gloo has no 16-bit integer type)
            pairs += [(img[n:2 * n].view(torch.int32), img[yown].view(torch.int32)) for img in (self.Zh, self.Zl)]
        else:
            pairs.append((self.Z[n:], self.Z[yown]))
        pairs += [(self.sqn[n:], self.sqn[yown]), (self.colpart, self.colpart_own)]
        if self._coalesce is None:
            self._coalesce = self._probe_coalescing(dist)
        if self._coalesce:  # one RCCL group launch for the three or four gathers instead of one launch each
            emulated = dist.get_world_size(self.group) != self.world
            with dist._coalescing_manager(group=self.group, device=self.dev, async_ops=True) as cm:
                for out, own in pairs:
                    dist.all_gather_into_tensor(own if emulated else out, own, group=self.group)
            return [cm]
        return [self._all_gather(dist, out, own) for out, own in pairs]

    def _probe_coalescing(self, dist):
        """Can this stack batch several all-gathers into one collective launch (torch's coalescing manager over RCCL's group
        calls)?  Tried ONCE, eagerly, on scratch tensors -- never for the first time inside a graph capture -- and only on the
        RCCL backend; any failure means "one launch per gather", never "no exchange"."""
        # (opt-in, VGAN_DP_COALESCE=1: on one GPU the coalesced form measures the same as separate launches -- 410.5 vs 400-411 us
        #  per emulated c4 shard -- and plain async all-gathers inside a graph capture are the better-trodden path for the first
        #  run on several GPUs)
        if os.environ.get("VGAN_DP_COALESCE", "0") != "1" or not self.data.is_cuda or torch.cuda.is_current_stream_capturing():
            return False
        try:
            if dist.get_backend(self.group) != "nccl" or not hasattr(dist, "_coalescing_manager"):
                return False
            size = dist.get_world_size(self.group)
            a, b = torch.zeros(size * 4, device=self.dev), torch.zeros(size * 2, dtype=torch.int64, device=self.dev)
            r = dist.get_rank(self.group)
            with dist._coalescing_manager(group=self.group, device=self.dev, async_ops=True) as cm:
                dist.all_gather_into_tensor(a, a[4 * r:4 * r + 4], group=self.group)
                dist.all_gather_into_tensor(b, b[2 * r:2 * r + 2], group=self.group)
            cm.wait()
            torch.cuda.synchronize()
            return True
        except Exception as e:  # noqa: BLE001
            import warnings
            warnings.warn(f"vgan_amd: coalesced all-gather is not available on this stack ({type(e).__name__}: {e}); one launch per gather")
            return False

    def _loss_backward_update_sharded(self, all_rows_here=False):
        """Gram (own Y rows x all columns + a share of the X-X triangle), backward, mask backward, M_4, all-reduce, chain
        backward, optimiser -- after `_forward_sharded` (or, all_rows_here: after the replicated front of the calibration
        step, which has produced every row on every rank: nothing to exchange)."""
        ops, n, nl, lo, d = self.ops, self.n, self.nl, self.lo, self.d
        dist = self._collect()
        works = []
        if all_rows_here:
            if self.bf3:
                ops.mmd_bf3_prepare(self.Z, 2 * n, d, self.Zh, self.Zl)
            self.colpart.zero_()
            ops.colmax_partial(self.S, 0, self.colpart[:ops.colmax_chunks(n) * d])
        else:
            works = self._exchange_front(dist)
        na = self.n_main

        def gram(t0, t1):
            if t1 <= t0:
                return
            if self.bf3:
                ops.mmd_gram_bf3(self.Zh, self.Zl, self.sqn, n, self.bw, self.tiles[t0:t1], self.Wh, self.Wl, n + lo, self.partial[t0:t1],
                                 tile=self.gram_tile, tail_ws=self.gram_tail_ws, rs_part=self.rs_part)
            else:
                ops.mmd_gram(self.Z, self.sqn, n, self.dp, self.bw, self.tiles[t0:t1], False, self.Wg, n + lo, self.partial[t0:t1])

        gram(0, na)                      # XY and X-X tiles: beside the all-gather
        for w in works:
            if w is not None:
                w.wait()
        gram(na, self.tiles.shape[0])    # YY tiles: every rank's Y rows
        if self._fin is None:
            self._fin = ops.finalize_job(self.partial, self.tiles, self.colpart, self.col_chunks, self.colkey, n, d,
                                         self.pen if self.rank == 0 else 0.0, self.stats, self.loss, self.loss_accum, self.accum_scale,
                                         self.step_counter)
        gstride = nl * self.dp
        if self.bf3:
            ops.mmd_backward_bf3_rm(self.Wh, self.Wl, self.Zh, self.Zl, 2 * n, self.Z, n + lo, nl, d, self.Z[lo:lo + nl], self.gU,
                                    self.bsplits, gstride, self._fin, mul_shift=self.center, tile=self.bwd_tile, rs_part=self.rs_part)
        else:
            ops.mmd_backward(self.Wg, self.Z, n + lo, nl, 2 * n, self.dp, self.Z[lo:lo + nl], self.gU, self.bsplits, gstride, self._fin,
                             mul_shift=self.center)
        ops.mask_backward(self.gU, self.S_own, self.colkey, self.pen, lo, self.dlogits, self.bsplits, gstride)
        self._generator_backward_update(dist)

    def _late_xx_job(self):
        """The X-X tiles the Gram launch had no slot for, as a job for the launch that carries them."""
        if self._xx_m4 is None:
            ntx = self.tiles.shape[0] - self.n_main
            self._xx_m4 = self.ops.xx_job(self.Zh, self.Zl, self.sqn, self.tiles[self.n_main:], self.bw,
                                          self.partial[self.n_main:self.n_main + ntx])
        return self._xx_m4

    def _step_body(self):
        if self.front_sharded:
            self._forward_sharded()
            self._loss_backward_update_sharded()
        else:
            self._forward()
            self._loss_backward_update()

    def step(self):
        """Runs one training step asynchronously.  The first step also calibrates the bandwidth."""
        if not self.has_bw:
            if self.overlap:  # no step ran before this one: the X half of its operand is produced here ...
                self._prefetch_x_operand()
            self._forward()  # (all rows on every rank, whatever the front mode: the calibration below needs them all)
            self._calibrate()
            if self.overlap or self.xx_ride:  # ... and its X-X sums here, with the fresh bandwidth
                self._xx_tiles()
                self._xx_primed = True
            if self.front_sharded:
                self._loss_backward_update_sharded(all_rows_here=True)
            else:
                self._loss_backward_update()
        elif self.use_graph and self.steps_done > 0:
            if self.graph is None:
                self._capture()
            if self.graph is not None:
                self.graph.replay()
            else:
                self._step_body()
        else:
            # eager: graphs off, or the very first step of an engine whose bandwidth was handed over (a second fit in one
            # process: the shared-RBF quirk) -- its first-ever launches and the one-off noise draw stay outside the capture
            if self.overlap and not self._xx_primed:
                self._prefetch_xx()
            self._step_body()
        self.steps_done += 1

    def run_steps(self, count):
        """`count` consecutive training steps of the current epoch table.  With the device noise stream nothing on the host
        changes between steps (the device-side step counter picks the batch and keys the noise), so steps are replayed in
        blocks of `steps_per_graph` from ONE graph launch: between two graph launches the GPU idles for ~8.5 us (MI355X,
        rocprofv3 kernel trace) -- 7 % of the c3 step, 16 % of the c1 step -- against ~1 us between kernels inside a graph.
        Host-provided noise (`set_noise`) is per step by nature: there, and while the engine is still eager, this is a loop
        over step()."""
        count = int(count)
        if count > 1 and self.noise_mode != "device":
            raise ValueError("run_steps needs the device noise stream: host-provided noise is set per step (set_noise + step)")
        m = self.steps_per_graph
        while count > 0:
            blk = min(count, m)
            if (blk > 1 and self.use_graph and self.has_bw and self.steps_done > 0 and self.noise_mode == "device" and
                    self.graph is not None):
                g = self._block_graph(blk)
                if g is not None:
                    g.replay()
                    self.steps_done += blk
                    count -= blk
                    continue
            self.step()
            count -= 1

    def _block_graph(self, steps):
        """The graph holding `steps` consecutive steps (captured at first use), or None.  An epoch of nb steps replays
        nb // 16 graphs of 16 and one of nb % 16; at most four block sizes are kept (a caller that asks for ever new
        remainders gets the one-step graph for them)."""
        g = self.graph_blocks.get(steps)
        if g is None and len(self.graph_blocks) < 4:
            g = self.graph_blocks[steps] = self._capture_graph(steps) or False
        if steps == self.steps_per_graph:
            self.graph_multi = g or None
        return g or None

    def _capture_graph(self, steps):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with no_gc_while_capturing(), torch.cuda.graph(g):
                for _ in range(steps):
                    self._step_body()
        except Exception as e:  # noqa: BLE001 -- any capture failure means "no graph", never "no training"
            import warnings
            warnings.warn(f"vgan_amd: HIP-graph capture of {steps} training step(s) failed ({type(e).__name__}: {e}); running eager launches")
            torch.cuda.synchronize()
            g = None
        # Several ranks must take the SAME path from here on (a replayed graph and eager launches issue the same collectives, but
        # a rank that fell back keeps launching while the others replay 16 steps at a time -- and a capture that failed on one
        # rank only would otherwise go unnoticed by the rest): agree on the outcome.  A capture executes nothing, so no rank has
        # a collective of the captured steps in flight here.
        if self.exchange and self.world > 1:
            dist = self._collect()
            ok = torch.tensor([1 if g is not None else 0], dtype=torch.int32, device=self.dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.group)
            if int(ok.item()) == 0:
                g = None
        return g  # capture does not execute: the steps that triggered it still have to run

    def _capture(self):
        """Captures one step into a HIP graph.  If the capture fails (e.g. a collective that cannot be captured on this
        stack) the engine keeps running the same launches eagerly, in this process."""
        self.graph = self._capture_graph(1)
        if self.graph is None:
            self.use_graph = False

    # ---- sampling (generate_subspaces) ---------------------------------------------------------
    def generator_logits(self, z):
        """Generator forward on caller noise [m, L] -> logits [m, d] (fresh buffers, eager, layer by layer)."""
        ops = self.ops
        h = z.to(device=self.dev, dtype=torch.float32).contiguous()
        for k in range(4):
            y = torch.empty(h.shape[0], self.W[k].shape[0], dtype=torch.float32, device=self.dev)
            ops.linear_forward(h, self.W[k], self.b[k], y)
            h = y
        return h

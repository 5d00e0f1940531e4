"""Schedule plan of the ``VGAN_no_kl`` step engine (trainer.py): which launches a step is made of, for a given shape.

Host only.  `Knobs.from_env` is the one place the construction-time ``VGAN_*`` environment variables are read; `plan_step`
turns the constructor's arguments and a `Knobs` into a frozen `StepPlan` without creating a device tensor, so the decision table
can be asked (and is pinned, tests/test_step_plan.py) for every workload without paying for the engine's ~60 buffers.
`NoKLStepEngine.__init__` runs it once and then only allocates.
"""
import dataclasses
import os
from typing import Optional, Union


def _round4(v):
    return (v + 3) // 4 * 4


def _launch_rounds(tiles, slots, can_split):
    """Time of a Gram launch of `tiles` tiles in units of one full round of `slots` resident workgroups.  A partial last round
    is NOT a whole round: with at most half the slots busy a tile runs about twice as fast (c5 wide tiles: 256 tiles 183 us,
    272 tiles 276, 384 tiles 290; c4: 101, 153, 159), and the wide kernel's K split of a short last round (gram_tail_ws) brings
    a remainder of up to an eighth / a quarter of the slots down to ~0.25 / ~0.4 of a round (c5: 16 tiles +28 us, 64 tiles +60)."""
    if tiles <= 0:
        return 0.0
    full, r = divmod(tiles, slots)
    if r == 0:
        return float(full)
    x = r / slots
    last = 0.55 if x <= 0.5 else 0.55 + 0.9 * (x - 0.5)
    if can_split and x <= 0.125:
        last = 0.25
    elif can_split and x <= 0.25:
        last = 0.4
    elif can_split and x <= 0.5:
        last = 0.5
    return full + last


def _best_boundary(n_main, total, slots, can_split):
    """First-part size <= n_main (tiles may only move to the SECOND launch, which runs after the all-gather and can take any tile)
    that minimises the modelled time of the two launches; the boundary moves only for a gain of at least 0.15 round (the
    model is not finer than that), and among equals as little as possible, so that most work stays beside the all-gather."""
    cost = lambda k: _launch_rounds(k, slots, can_split) + _launch_rounds(total - k, slots, can_split)
    best, best_cost = n_main, cost(n_main)
    for k in range(n_main - 1, max(n_main - slots, 0), -1):
        c = cost(k)
        if c < best_cost - 1e-9 and c <= cost(n_main) - 0.15:
            best, best_cost = k, c
    return best


CHAIN_KPARTS_AUTO = 4  # the measured winner of {1, 2, 4, 8} for both launches it applies to


def chain_kparts(want, tiles, k, chain_flops=False):
    """Workgroups per 32 x 32 output tile for one long-K launch of the collapsed chain's backward (in-launch K split,
    vgan_linear_backward_params_ksplit / vgan_gemm_grouped_ksplit).  `tiles` = the launch's 32 x 32 output tiles, `k` = its
    shortest contraction; `want` = VGAN_CHAIN_KPARTS: "auto", or 1 | 2 | 4 | 8 to force a count (measurement knob).
    "auto" splits only where it was measured to win (MI355X, profiles/README.md, Round 5): a launch of 32-64 tiles -- a fifth of
    the chip -- with a contraction of 768 or more, i.e. the c3 step's M_4 (50 tiles, K = 1024) and its first chain-backward
    launch (48 tiles, K = 788).  Everything else stays at 1: the c1 / c2 chains (1-12 tiles, K <= 512: not measured, and near the
    ~5 us floor of a dependent launch already), the flop-minimal association of c4 / c5 (hundreds of tiles; its long products use slabs of C)."""
    if want != "auto":
        parts = int(want)
        if parts not in (1, 2, 4, 8):
            raise ValueError(f"VGAN_CHAIN_KPARTS must be auto, 1, 2, 4 or 8, got {want!r}")
        return parts
    if chain_flops or not (32 <= tiles <= 64 and k >= 768):
        return 1
    return CHAIN_KPARTS_AUTO


def _knob(var, default, parse=str):
    """A Knobs field: its environment variable, the default as the variable would spell it, and how a spelling is read."""
    return dataclasses.field(default=None if default is None else parse(default), metadata=dict(var=var, default=default, parse=parse))


_is_1 = lambda v: v == "1"    # on only when spelled 1
_not_0 = lambda v: v != "0"   # off only when spelled 0


@dataclasses.dataclass(frozen=True)
class Knobs:
    """The construction-time measurement knobs of the step engine, one field per environment variable.  Defaults are the
    measured winners; a constructor argument, where one exists, wins over its knob.  The library reads no environment.

    variable              values (default first)              forces                                                     measured in
    VGAN_GENERATOR        collapsed | layered                 the generator as a chain in homogeneous coordinates, or     DESIGN.md 4
                                                              layer by layer
    VGAN_FUSE_UPDATE      0 | 1                               Adadelta in the epilogue of the last chain launch (depth    DESIGN.md 5, Round 2 table
                                                              association only)
    VGAN_DP_FRONT         auto | replicated | sharded         who runs the O(n d) front of a data-parallel step           DESIGN.md 6
    VGAN_CHAIN_ASSOC      auto | depth | flops                suffix products (fewer dependent launches) or the           DESIGN.md 4
                                                              flop-minimal chain
    VGAN_CHAIN_SPLITK     1 | other                           K slices (slabs of C) of the flop-minimal chain's long      DESIGN.md 4
                                                              products on / off
    VGAN_MMD_PRECISION    auto | fp32 | bf16x3                Gram / backward products on the fp32 or the bf16 MFMA       DESIGN.md 4, profiles/r02_precision_probe.txt
    VGAN_BWD_TILE         0 | 64 | 128 | 256                  tile of the bf16x3 backward (0: the library's choice)       DESIGN.md 4
    VGAN_BWD_OPERAND      rowmajor | transposed               the backward reads the Gram's images, or transposed copies  DESIGN.md 3, 4
    VGAN_BWD_SPLITS       (auto) | count                      split-K slabs of the backward product                       DESIGN.md 4
    VGAN_FUSED_PREPARE    1 | other                           mask forward fused with the bf16x3 operand split            DESIGN.md 4
    VGAN_CHAIN_IN_MASK    0 | 1                               logits product inside the mask / projection launch          DESIGN.md 5, Round 2 table
    VGAN_LOGITS_2STAGE    0 | 1                               logits as the second half of a two-stage tile               profiles/README.md, Round 3
    VGAN_GRAM_TILE        auto | 128 | 256 | other (= 64)     tile of the bf16x3 Gram (256 = 256 x 128 loader-wave tiles) DESIGN.md 4
    VGAN_GRAM_TAIL        1 | 0                               K split of the wide Gram's short last round                 profiles/README.md, Round 3
    VGAN_RS_FROM_GRAM     1 | 0                               row sums of W from the wide Gram's epilogue                 profiles/README.md, Round 3
    VGAN_OVERLAP          (unset = 0) | 1 | 0 | serial        next batch's X operand and X-X tiles behind the step's      DESIGN.md 5, Round 2 table,
                                                              tail, on a side stream (serial: on the one stream)          profiles/r02_overlap_schedules.txt
    VGAN_XX_RIDE          0 | 1                               X-X tiles ride in the mask / projection launch              DESIGN.md 5, Round 2 table
    VGAN_XX_IN_M4         1 | other                           X-X tiles the Gram launch has no slot for run later in the  DESIGN.md 5, Round 2 table
                                                              step (split step tail)
    VGAN_GRAM_SLOTS       512 | count                         resident workgroups the Gram launch is planned for (tests   DESIGN.md 5, Round 2 table
                                                              force a split at small sizes with it)
    VGAN_XX_LATE          backward | other (= m4)             carrier of the late X-X tiles                               DESIGN.md 5, Round 2 table
    VGAN_CHAIN_KPARTS     auto | 1 | 2 | 4 | 8                workgroups per tile of the two long-K chain launches        profiles/README.md, Round 5
    VGAN_Z_FP32           0 | 1                               keeps the fp32 operand copy and the reading backward        profiles/README.md, Round 4

    (VGAN_FEED_DIRECT, VGAN_DP_COALESCE and VGAN_FIT_SYNC_EACH_EPOCH are call-time switches, read where they act.)"""
    generator: str = _knob("VGAN_GENERATOR", "collapsed")
    fuse_update: bool = _knob("VGAN_FUSE_UPDATE", "0", _is_1)
    dp_front: str = _knob("VGAN_DP_FRONT", "auto")
    chain_assoc: str = _knob("VGAN_CHAIN_ASSOC", "auto")
    chain_splitk: bool = _knob("VGAN_CHAIN_SPLITK", "1", _is_1)
    mmd_precision: str = _knob("VGAN_MMD_PRECISION", "auto")
    bwd_tile: int = _knob("VGAN_BWD_TILE", "0", int)
    bwd_transposed: bool = _knob("VGAN_BWD_OPERAND", "rowmajor", lambda v: v == "transposed")
    bwd_splits: Optional[int] = _knob("VGAN_BWD_SPLITS", None, lambda v: None if v is None else int(v))  # None: the shape's own count
    fused_prepare: bool = _knob("VGAN_FUSED_PREPARE", "1", _is_1)
    chain_in_mask: bool = _knob("VGAN_CHAIN_IN_MASK", "0", _is_1)
    logits_2stage: bool = _knob("VGAN_LOGITS_2STAGE", "0", _is_1)
    gram_tile: str = _knob("VGAN_GRAM_TILE", "auto")
    gram_tail: bool = _knob("VGAN_GRAM_TAIL", "1", _not_0)
    rs_from_gram: bool = _knob("VGAN_RS_FROM_GRAM", "1", _not_0)
    overlap: Union[None, bool, str] = _knob("VGAN_OVERLAP", None, lambda v: {"1": True, "0": False}.get(v, v))  # as overlap_exchange
    xx_ride: bool = _knob("VGAN_XX_RIDE", "0", _is_1)
    xx_in_m4: bool = _knob("VGAN_XX_IN_M4", "1", _is_1)
    gram_slots: int = _knob("VGAN_GRAM_SLOTS", "512", int)
    xx_late_in_backward: bool = _knob("VGAN_XX_LATE", "backward", lambda v: v == "backward")
    chain_kparts: str = _knob("VGAN_CHAIN_KPARTS", "auto")  # (validated where it applies: chain_kparts)
    z_fp32: bool = _knob("VGAN_Z_FP32", "0", _is_1)

    @classmethod
    def from_env(cls, environ=os.environ):
        """The knobs as `environ` sets them: the only place these variables are read."""
        return cls(**{f.name: f.metadata["parse"](environ.get(f.metadata["var"], f.metadata["default"])) for f in dataclasses.fields(cls)})


@dataclasses.dataclass(frozen=True)
class StepPlan:
    """Every decision the step methods and bench.py read, and the derived sizes the allocator needs."""
    mode: str                   # "collapsed" | "layered"
    exchange: bool              # the data-parallel path, collectives included
    front_sharded: bool
    fuse_update: bool
    chain_flops: bool
    fwd_split: Optional[dict]   # flop-minimal chain: K slices of At_k = Wt_k At_{k-1} / M_{k-1} = Wt_k^T M_k, by k
    bwd_split: Optional[dict]
    precision: str              # "fp32" | "bf16x3"
    bf3: bool
    bwd_tile: int
    splits: int                 # row slabs of the layered weight gradients
    bsplits: int                # split-K slabs of the MMD backward
    rm_backward: bool
    fused_prepare: bool
    chain_in_mask: bool
    two_stage_logits: bool
    gram_tile: int
    gram_tail: bool             # lend the wide Gram its tail workspace (gram_tail_ws)
    rs_from_gram: bool          # keep the wide Gram's per-slot row sums (rs_part)
    overlap: bool
    side_stream: bool           # overlap on a stream of its own (a HIP device permitting)
    x_ahead: bool
    xx_ride: bool
    xx_in_m4: bool
    xx_late_in_backward: bool
    tile_split: Optional[str]   # None | "xx_last" | "yy_last": order of the tile table
    n_tiles: int
    n_main: int                 # tiles of the step's (first) Gram launch
    cal_shares_tiles: bool      # the calibration launch runs the step's own table
    m4_kparts: int
    tn_kparts: int
    lean: bool
    col_chunks: int
    nl: int
    lo: int
    dp: int
    e: list                     # padded homogeneous widths
    kp: int                     # bf16x3 images: padded feature / row counts
    kn: int


def plan_step(ops, *, n, d, data_stride, latent, widths, world, rank, force_exchange, generator_mode, mmd_precision,
              overlap_exchange, fuse_update, front, chain_assoc, knobs, host_tables=None):
    """The schedule of a step for the constructor's arguments (NoKLStepEngine.__init__) and `knobs`.  `ops` answers host queries
    only (tile counts, the library's tile and support rules, the provider's capabilities); nothing is allocated on a device.
    `host_tables`: a dict that receives the host tile tables counted on the way, by (tile, split), so that a caller that goes on
    to allocate does not build the chosen one a second time."""
    assert widths[0] == latent and len(widths) == 5
    # take the data-parallel exchange path (collectives included) even with one rank: lets a single GPU exercise it
    exchange = world > 1 or bool(force_exchange)
    if n % world != 0:
        raise ValueError(f"global batch {n} must be divisible by the number of ranks {world}")
    nl = n // world
    lo, dp = rank * nl, _round4(d)
    mode = generator_mode or knobs.generator
    if mode not in ("collapsed", "layered"):
        raise ValueError(f"generator_mode must be 'collapsed' or 'layered', got {mode!r}")
    collapsed = mode == "collapsed"
    # collapsed mode, opt-in (VGAN_FUSE_UPDATE=1): Adadelta in the epilogue of the last chain launch instead of a launch of
    # its own.  Built, parity-tested and measured on MI355X at c3 (same box, alternating runs): 8 358-8 444 steps/s fused vs
    # 8 424-8 529 separate -- the 127 tiles of that launch stream the 8 MB of optimiser state with far less memory-level
    # parallelism than the 1 600 workgroups of the streaming kernel (12.5 us vs 5.1 + 5.3 us), which costs more than the
    # removed launch boundary returns.  Kept off by default.
    fuse_update = knobs.fuse_update if fuse_update is None else bool(fuse_update)
    # Data-parallel FRONT of the step (generator forward, mask, projection, operand split -- O(n d) work):
    #   "replicated"  every rank produces all n rows of U and Y itself (module docstring): no exchange before the Gram; right
    #                 while the front is a handful of microseconds (c3: ~10 us);
    #   "sharded"     SURVEY 8e steps 1-2: a rank runs the logits product, mask / projection and operand split for ITS n/G rows
    #                 only and the ranks all-gather the Y rows of the operand (split images or fp32 rows, their norms, and the
    #                 column arg-max keys of the rows, which the step tail folds by max exactly like its own chunks).  The X half
    #                 of the operand needs no parameter, so every rank gathers it from the resident data set itself, and the
    #                 tiles that read no other rank's Y rows (XY and X-X: ~60 % of a rank's table) run BESIDE the all-gather.
    #   "auto"        sharded when there is an exchange at all and n d >= 2^22 (c4 / c5; at those sizes the replicated front
    #                 is 25-40 % of a 1/8 shard's step).
    # Replicas stay bit-identical (every rank sees the same gathered bytes and the same all-reduced M_4); results agree with
    # the replicated front to fp32 rounding of the logits product (its tile shape follows the row count).
    want_front = front or knobs.dp_front
    if want_front not in ("auto", "replicated", "sharded"):
        raise ValueError(f"front must be 'auto', 'replicated' or 'sharded', got {want_front!r}")
    if want_front == "sharded" and not (exchange and collapsed):
        raise ValueError("front='sharded' needs a data-parallel engine (world > 1 or force_exchange) with the collapsed generator")
    front_sharded = exchange and collapsed and (want_front == "sharded" or (want_front == "auto" and n * d >= (1 << 22)))

    # products that contract over the batch rows are cut into row slices ("slabs", summed in fixed order)
    # so that a launch with a small output still fills the chip
    splits = max(1, min(8, nl // 128))
    e = [_round4(w + 1) for w in widths]  # padded homogeneous widths
    chain_flops, fwd_split, bwd_split = False, None, None
    if collapsed:
        # Association of the chain.  "depth" (suffix products, 3 + 2 dependent launches) buys latency with flops -- the
        # product B_3 = Wt_4 Wt_3 alone is 2 e4 e3 e2 flop, 17 GFLOP of the 37 the chain costs at c5 (555 us of an 8.2 ms
        # step, replicated on every rank of a data-parallel run).  "flops" keeps every product an [e_k, e_{k-1}] x
        # [e_{k-1}, e0] one (At_k = Wt_k At_{k-1}, M_{k-1} = Wt_k^T M_k): 3 + 4 dependent launches, 17 GFLOP at c5.
        # "auto": flops once the suffix product passes 1 GFLOP (c4: 2.2, c3: 0.12).
        want_assoc = chain_assoc or knobs.chain_assoc
        if want_assoc not in ("auto", "depth", "flops"):
            raise ValueError(f"chain_assoc must be 'auto', 'depth' or 'flops', got {want_assoc!r}")
        chain_flops = want_assoc == "flops" or (want_assoc == "auto" and 2.0 * e[4] * e[3] * e[2] >= 1e9)
    if chain_flops:
        fuse_update = False  # (the fused optimiser epilogue is written for the depth-first launches)
        # Products with a long contraction over few 64 x 64 output tiles (c5: M_3 = Wt_4^T M_4 is 165 tiles of K = 4100 on
        # 256 CUs, 116 us for 4.4 GFLOP) are cut into K slices run by different workgroups -- ~1000 work items per
        # product -- whose partial slabs a small launch sums in fixed order (no atomics: replicas stay bit-identical).
        def split_of(m, n_, k):
            t64 = ((m + 63) // 64) * ((n_ + 63) // 64)
            return 1 if (2.0 * m * n_ * k < 2.5e8 or not knobs.chain_splitk) else max(1, min(8, 1024 // t64, k // 256))
        fwd_split = {k: split_of(e[k], e[0], e[k - 1]) for k in (2, 3, 4)}       # At_k = Wt_k At_{k-1}
        bwd_split = {k: split_of(e[k - 1], e[0], e[k]) for k in (4, 3, 2)}       # M_{k-1} = Wt_k^T M_k

    # MMD arithmetic.  "fp32": Gram/backward products on the fp32 MFMA (default for small problems); "bf16x3": split-bf16
    # operands on the (16x faster) bf16 MFMA, three products per term, fp32 accumulate (see csrc/mmd_bf16.hip: ~3e-7 relative on
    # a Gram entry at K = 784, a third of the time; parity tests hold it to the same 1e-4 bar).  "auto" keeps fp32 for small
    # problems, where the operand-preparation launch would not pay.
    precision = mmd_precision or knobs.mmd_precision
    if precision not in ("auto", "fp32", "bf16x3"):
        raise ValueError(f"mmd_precision must be 'auto', 'fp32' or 'bf16x3', got {precision!r}")
    if precision == "auto":
        precision = "bf16x3" if 2 * n * d >= (1 << 20) else "fp32"
    bf3 = precision == "bf16x3"
    bwd_tile = knobs.bwd_tile  # measurement knob: force the 64- / 128-wide bf16x3 backward tile
    # The backward product W . Z reads the SAME row-major images as the Gram (vgan_mmd_backward_bf3_rm: B fragments by
    # transposed LDS reads), so the operand preparation writes no transposed copy of Z (6.6 MB of scattered 16-byte stores
    # per step at c3).  VGAN_BWD_OPERAND=transposed keeps the round-1 form (ZTh / ZTl) for measurement.
    rm_backward = not bf3 or front_sharded or not knobs.bwd_transposed
    # The backward GEMM contracts over the 2n rows of Z; it can be sliced into row slabs that the mask-backward kernel
    # sums.  Measured at c3: 2 slabs pay for the split-bf16 kernel (24.3 vs 29.6 us; 3 and 4 spill into a second round
    # of workgroups), none do for the fp32 kernel.  Small problems have only a handful of output tiles with a long K
    # loop each (c2: 24 tiles, 26 us of an 84 us step), so the slab count also grows until the launch fills the chip.
    out_tiles = ((nl + 63) // 64) * ((d + 63) // 64)
    # (a slab keeps at least one 64-deep K tile: at c1 -- two output tiles, K = 256 -- four slabs of one K tile beat one
    #  workgroup looping over four, 23.5 k vs 21.9 k steps/s; 8 and 16 slabs at c2: the consumer's slab loop costs more than it saves)
    auto_splits = max(2 if bf3 else 1, min(4, 256 // max(out_tiles, 1), max(1, (2 * n) // 64)))
    # (the 256 x 128 loader-wave tiles of c4 / c5 fill the chip without slabs: c5 3.27 ms with two slabs, 3.16 with one)
    if bf3 and rm_backward and bwd_tile in (0, 256) and ops.mmd_backward_bf3_tile(nl, d, 1, bwd_tile) == 256:
        auto_splits = 1
    bsplits = max(1, auto_splits if knobs.bwd_splits is None else knobs.bwd_splits)
    bwd_edge = ops.mmd_backward_bf3_tile(nl, d, bsplits, bwd_tile) if bf3 else 0  # tile edge the bf16x3 backward will run
    fused_prepare = bf3 and not front_sharded and ops.bf3_fusable(n, d, d, data_stride, dp) and knobs.fused_prepare
    # collapsed generator, opt-in (VGAN_CHAIN_IN_MASK=1): the logits product inside the mask / projection launch (one wave per
    # batch row, the row's logits live in its registers anyway): one launch and 2 n d x 4 bytes of traffic less per step.
    # MEASURED (MI355X, c3, same box, alternating runs): 8 029-8 038 steps/s fused vs 8 371-8 455 separate (fp32 mode 5 873 vs
    # 6 316).  Every workgroup has to stage all of At_4 (163 KB, transposed through LDS in four chunks, each a dependent
    # global load + barrier) for its 8 rows: the carrying launch grows from 9.5 to 21.8 us, more than the 5.2 us launch it
    # replaces.  Off by default.
    chain_in_mask = (collapsed and not front_sharded and ops.chain_fusable(n, d, data_stride, dp) and
                     (not bf3 or fused_prepare) and knobs.chain_in_mask)
    # collapsed generator, depth-first association, opt-in (VGAN_LOGITS_2STAGE=1): the logits product as the second half of a
    # two-stage tile (see _generator_forward) -- one dependent launch less per step.  MEASURED (MI355X, c3, same box,
    # alternating runs): 9 285, 9 265 steps/s against 9 702, 9 715 with the three-launch forward (fp32 mode 6 324-6 337 vs
    # 6 522-6 544): the two carrying launches grow by more than the 5.1 us launch they replace (a two-stage tile is three
    # dependent K loops and a workgroup barrier deep; the logits as a K = 200 product over 208 tiles is no longer a 5 us
    # launch's worth riding in a 6.8 us one).  Off by default.
    two_stage_logits = collapsed and not chain_flops and not chain_in_mask and not front_sharded and knobs.logits_2stage

    def count_tiles(tile, split=None):
        """(tiles, tiles of the first part) of this rank's table, built on the host."""
        table = ops.build_tiles(n, 1, rank, world, device="cpu", tile=tile, split=split)
        if host_tables is not None:
            host_tables[tile, split] = table
        return (table[0].shape[0], table[1]) if split else (len(table), len(table))

    # Gram tile edge: the split-bf16 Gram has a 128x128 variant (half the L2 -> LDS bytes per flop, one 512-thread
    # workgroup per CU).  Measured: c5 330 vs 273 TFLOP/s algorithmic, c3 (136 tiles of 128) no gain (26.3 vs 25.6 us),
    # so it is used once its table fills the chip twice over and the row shard is a whole number of tiles.
    gram_tile = 64
    # ... and a 256 x 128 variant with dedicated loader waves (csrc/gemm_bf3w.hpp: 3/4 of the fill bytes per flop, three
    # K stages in LDS, v_mfma_f32_16x16x32_bf16; main loop +17-19 % over the 128 x 128 one on warm operands), used once ITS
    # table fills the chip twice over (c4: 1 056 tiles, c5: 4 160)
    for edge in (128, 256):
        if bf3 and nl % edge == 0 and knobs.gram_tile in ("auto", str(edge)):
            if knobs.gram_tile == str(edge) or count_tiles(edge)[0] >= 512:
                gram_tile = edge
    small_tiles = gram_tile == 64
    # one 768-thread workgroup holds a CU, so a table runs in rounds of 256 tiles; the library splits a short last round over
    # K when it is lent this workspace (include/vgan_hip.h, tail_ws: c4's 1 040 tiles = 4 rounds + 16 tiles)
    gram_tail = gram_tile == 256 and knobs.gram_tail
    # ... and its epilogue leaves the row sums of W per 128-column slot, which the 256 x 128 backward kernel folds instead of
    # summing W's rows from LDS with its loader waves (-5 % of that launch at c5)
    rs_from_gram = gram_tile == 256 and rm_backward and n % 128 == 0 and knobs.rs_from_gram and bwd_edge == 256

    # Overlap of the step's tail with the only work of the NEXT step that needs no updated parameter: the X half of its
    # operand (gather, centre, split) and the X-X tiles of its Gram, which feed nothing but the reported loss.  They run on
    # a side stream that forks right after the MMD backward launch (whose riding step tail has advanced the batch cursor)
    # and joins at the end of the step -- concurrent with the mask backward, the M_4 contraction, the gradient all-reduce of
    # a data-parallel run, the chain backward and the optimiser, all of which are small launches that leave most CUs
    # idle.  The table is laid out as [XY and YY tiles | XX tiles]: the step's Gram launch covers the first part (392
    # instead of 528 tiles at n = 1024: no second round on the 512 resident slots), the side launch the second, and the
    # step tail folds both (one table, one partial buffer).  overlap_exchange=False: the plain one-stream schedule with
    # the XX tiles inside the Gram launch; "serial": the overlapped schedule's launches on ONE stream (measurement aid).
    if overlap_exchange is None:
        overlap_exchange = knobs.overlap  # measurement knob: 1 | 0 | serial
    # MEASURED (MI355X, c3, same box, profiles/r02_overlap_schedules.txt): the side-stream schedule LOSES on this stack --
    # 6 843-6 972 steps/s against 8 259-8 529 plain on one GPU; emulated 1/8 shard 120 us against 87 (plain) and 105 (same
    # launches on one stream).  The Gram does drop from 24.2 to 14.2 us without its 136 X-X tiles, but two kernels running
    # side by side inside the graph slow each other (M_4 product 8.5 -> 13.0 us, mask backward 5.1 -> 6.9) and the fork /
    # join is not free.  The default is therefore the plain schedule; the option stays for stacks where streams are cheap.
    overlap = False if overlap_exchange is None else bool(overlap_exchange)
    if front_sharded and overlap:
        raise ValueError("overlap_exchange and front='sharded' are two schedules of the same exchange: choose one")
    side_stream = overlap and overlap_exchange != "serial"
    # with the X half of the operand produced ahead of the step, the mask / projection launch writes the Y half only
    x_ahead = overlap and rm_backward
    # the step as one stream of launches with nothing exchanged or prefetched around its Gram: what every rider below needs
    plain_schedule = not overlap and not front_sharded

    # bf16x3 mode, fused forward: the X-X tiles (sums only, independent of everything the step computes) ride in the mask /
    # projection launch as surplus workgroups, reading the batch's rows through the index table from split images of the
    # whole data set prepared ONCE by the engine (csrc/mmd_xx.hpp).  The Gram launch keeps the XY and YY tiles: 392 instead of
    # 528 at n = 1024, one round on the chip's 512 resident slots instead of two.  Riding wants every workgroup of the launch
    # resident at once (a tile's workgroup holds 74 KB of LDS: two per CU).
    # MEASURED (MI355X, c3, same box, alternating runs): 8 266-8 319 steps/s riding vs 8 399-8 512 with the tiles inside the
    # Gram launch.  The Gram does shrink (24.2 -> 17.5 us) but the carrying launch grows from 9.4 to 18.3 us: gathered from
    # the data set's images the tiles' operand is HBM-cold (in the Gram it is the L2-hot image the forward has just
    # written) and their K loop becomes latency-bound.  Opt-in (VGAN_XX_RIDE=1), off by default.
    xx_ride = False
    if fused_prepare and small_tiles and plain_schedule and rm_backward and knobs.xx_ride:
        total, first = count_tiles(64, "xx_last")
        xx_tiles = total - first
        xx_ride = xx_tiles > 0 and 8 * ((n // 8 + 7) // 8) + xx_tiles <= 512  # two workgroups per CU (74 KB of LDS each)
    # X-X tiles outside the Gram launch, on a warm operand (the step's own Zh / Zl X half, identity row map).  `xx_in_m4` =
    # "some X-X tiles are computed LATER in the step than the launch that carries the step tail" (the tail is then split);
    # their carrier is the MMD backward launch when it has room (`xx_late_in_backward`), else the M_4 launch.
    xx_in_m4 = (bf3 and collapsed and small_tiles and plain_schedule and not xx_ride and
                ops.linear_backward_params_xx_supported(nl, e[0], dp) and knobs.xx_in_m4)
    if front_sharded:
        # [XY and X-X tiles | YY tiles]: the first part reads this rank's own Y rows and X columns only and runs while the
        # other ranks' Y rows are still on their way (`_loss_backward_update_sharded`)
        tile_split = "yy_last"
        n_tiles, n_main = count_tiles(gram_tile, tile_split)
        # Both launches run in rounds of `slots` resident workgroups (128-wide tiles: one 512-thread workgroup per CU; 64-wide:
        # two), so a first part of 3 x 256 + 4 tiles pays a fourth round for the four (c5, 8 ranks: 772 + 484 tiles, 352 + 198
        # us against ~100 us per round).  The boundary may move DOWN freely -- the second launch runs after the all-gather and
        # can take any tile -- so the tail of the first part goes over when the second part has free slots for it.
        # `_best_boundary` puts it where the modelled time of the two launches is least (128-wide tiles, c5, 8 ranks:
        # 772 + 484 -> 768 + 488).
        slots = 256 if gram_tile >= 128 else (512 if bf3 else 1024)  # (fp32 kernel: 36 KB of LDS, four workgroups per CU)
        n_main = _best_boundary(n_main, n_tiles, slots, gram_tail)
    elif overlap or xx_ride or xx_in_m4:
        tile_split = "xx_last"
        n_tiles, n_main = count_tiles(gram_tile, tile_split)
        if xx_in_m4:
            # ... but only the X-X tiles the Gram launch has no free slot for: at two 74 KB workgroups per CU the chip holds
            # 512 tiles at once, and a CU works through two of them in 13.3-14.1 us whether its neighbour has one or two
            # (tools/ablate_bf3_glds.hip: 392 tiles 13.3 us, 512 tiles 14.1 us).  c3: 392 XY + YY tiles + 120 of the 136 X-X
            # tiles in the Gram launch, 16 left over.
            n_main = min(n_tiles, max(n_main, knobs.gram_slots))  # (tests force a split at small sizes with VGAN_GRAM_SLOTS)
            xx_in_m4 = n_main < n_tiles  # everything fits the one launch: no carrier, one tail
    else:
        tile_split = None
        n_tiles, n_main = count_tiles(gram_tile)
    # The few X-X tiles left over (c3: 16) ride in the MMD BACKWARD launch when it has free slots for them: that launch fills
    # 416 of the 512 slots for 25 us, so eight-microsecond tiles on the other slots cost nothing, whereas behind M_4 even 16
    # tiles stretch the launch from 8.5 to 12.1 us (a lone tile's latency, not their number).  The late half of the split
    # tail (first chain launch of the backward) picks their sums up either way.
    bwd_wgs = ((d + 63) // 64) * ((nl + 63) // 64) * bsplits + 1
    xx_late_in_backward = (xx_in_m4 and rm_backward and knobs.xx_late_in_backward and bwd_edge == 64 and
                           n_tiles - n_main <= 512 - bwd_wgs)
    # the first-call bandwidth needs sum(L) over ALL pairs: computed by every rank from the full table (no collective)
    # (the calibration launch is the fp32 kernel: 64-wide tiles)
    cal_shares_tiles = world == 1 and small_tiles and plain_schedule and not xx_ride and not xx_in_m4

    # In-launch K split of the two long-K launches of the chain's backward (chain_kparts): M_4 = dlogits^T [z|1] unless the
    # X-X tiles ride behind it, and {M_3, M_2, M_1} on the depth association.
    m4_kparts = tn_kparts = 1
    if collapsed and getattr(ops, "chain_ksplit", False):
        t32 = lambda rows, cols: ((rows + 31) // 32) * ((cols + 31) // 32)
        if not (xx_in_m4 and not xx_late_in_backward):
            m4_kparts = chain_kparts(knobs.chain_kparts, t32(dp, e[0]), nl, chain_flops)
        tn_tiles = sum(t32(e[k], e[0]) for k in (3, 2, 1))
        if not chain_flops and e[4] >= 96 and tn_tiles <= 256:  # (the library's 16-wave grouped launch: what can be split)
            tn_kparts = chain_kparts(knobs.chain_kparts, tn_tiles, e[4])
    # The default bf16x3 step (fused forward, 64-wide Gram and backward tiles, row-major backward operand, one rank, no
    # side stream) keeps no fp32 copy of its operand (`lean`).  The Gram reads the split images, and the only reader of Z
    # in the step was the backward's epilogue; it now forms those two numbers per element from the data row, S and the
    # centre -- the same bits (vgan_mmd_backward_bf3_rm_rebuild).  The forward writes `xrow`, the batch's data-set rows,
    # because the step tail that rides in the backward launch advances the batch cursor while that launch runs.  Z is
    # still written by every step taken before the bandwidth exists (the calibration reads it).  VGAN_Z_FP32=1 keeps the
    # fp32 copy and the reading backward, for A/B runs.  MEASURED (MI355X, c3, alternating runs on one box,
    # profiles/README.md): 0.1044 -> 0.1010 ms per step; the backward launch 25.9 -> 22.9 us, the forward 9.1 -> 8.7.
    # (an ops provider says it has these launches with `bf3_rebuild`: a stand-in without them runs the step as before)
    lean = (getattr(ops, "bf3_rebuild", False) and fused_prepare and small_tiles and rm_backward and world == 1 and
            plain_schedule and bwd_edge == 64 and not knobs.z_fp32)
    # column arg-max keys of topk(U, 1, 0): per 64-row chunk, folded by max in the step tail.  Sharded front: one slice of
    # chunks per rank (its rows' keys carry GLOBAL row numbers), all-gathered with the Y rows; the tail folds them all.
    col_chunks = (world * ops.colmax_chunks(nl)) if front_sharded else ops.colmax_chunks(n)
    return StepPlan(mode=mode, exchange=exchange, front_sharded=front_sharded, fuse_update=fuse_update, chain_flops=chain_flops,
                    fwd_split=fwd_split, bwd_split=bwd_split, precision=precision, bf3=bf3, bwd_tile=bwd_tile, splits=splits,
                    bsplits=bsplits, rm_backward=rm_backward, fused_prepare=fused_prepare, chain_in_mask=chain_in_mask,
                    two_stage_logits=two_stage_logits, gram_tile=gram_tile, gram_tail=gram_tail, rs_from_gram=rs_from_gram,
                    overlap=overlap, side_stream=side_stream, x_ahead=x_ahead, xx_ride=xx_ride, xx_in_m4=xx_in_m4,
                    xx_late_in_backward=xx_late_in_backward, tile_split=tile_split, n_tiles=n_tiles, n_main=n_main,
                    cal_shares_tiles=cal_shares_tiles, m4_kparts=m4_kparts, tn_kparts=tn_kparts, lean=lean, col_chunks=col_chunks,
                    nl=nl, lo=lo, dp=dp, e=e, kp=(d + 63) // 64 * 64, kn=(2 * n + 63) // 64 * 64)
